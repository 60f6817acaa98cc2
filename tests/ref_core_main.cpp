// ref_core_main.cpp — the host forms of the reference gather's core and of the .fai event core (cutesv_amd/csrc/ref_core.h, RefOneLane) over a corpus file, as a
// stand-alone program: tests/test_bgzf_reference.py builds it with -fsanitize=address,undefined and compares what it writes with
// csv_ref_gather_host's bytes.  The blocks' bytes stand in one heap block of exactly their size and the output in one of exactly
// the ranges' size, so a read or a write one byte outside either is the sanitizer's to report.
//
// And the event core (fai_events_host, FaiStream): the windows of a text, each a heap block of exactly its size, as event rows in a
// heap block of exactly their count, and the index assembled from them beside the index of the same windows fed as bytes.
//
//   ref_core_main events WINDOWS
//   WINDOWS: u32 windows, then per window u32 bytes and the bytes
//   stdout:  per window "window K rows N", its rows "start bytes bases", then "rows" / "bytes" and the entries of either index
//            ("name length offset line_bases line_width") or "refused"
//
//   ref_core_main CORPUS OUT
//   CORPUS: u32 blocks, then per block i64 uoff, u32 bytes and the bytes; u32 ranges, then per range i64 base_off, i32 line_bases,
//           i32 line_width, i64 beg, i64 end
//   OUT:    the bases of the covered ranges, in order, back to back
//   stdout: "tile N", then per range "ordinal covered bases"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../cutesv_amd/csrc/ref_core.h"

using namespace csv;

template <class T> static T take(const std::vector<unsigned char>& f, size_t& o)
{
    T v;
    if (o + sizeof v > f.size()) { fprintf(stderr, "the corpus is cut short\n"); exit(2); }
    memcpy(&v, f.data() + o, sizeof v);
    o += sizeof v;
    return v;
}

static void print_index(const char* what, FaiStream& s)
{
    printf("%s\n", what);
    if (!s.finish()) { printf("refused\n"); return; }
    for (const FaiStream::Entry& e : s.ent)
        printf("%.*s %lld %lld %d %d\n", e.name_len, s.names.data() + e.name_off, e.length, e.offset, e.lb, e.lw);
}

static int events(const std::vector<unsigned char>& f)
{
    size_t o = 0;
    const uint32_t nw = take<uint32_t>(f, o);
    FaiStream by_rows, by_bytes;
    bool rows_ok = true;
    for (uint32_t k = 0; k < nw; k++) {
        const uint32_t n = take<uint32_t>(f, o);
        if (o + n > f.size()) { fprintf(stderr, "the windows are cut short\n"); return 2; }
        uint8_t* d = (uint8_t*)malloc(n ? n : 1);                            // exactly the window
        memcpy(d, f.data() + o, n);
        o += n;
        const FaiCarry c = by_rows.carry();
        FaiCarry tail;
        const ref_i64 need = fai_events_host(d, n, by_rows.fed, c, nullptr, 0, &tail);
        FaiRow* rows = (FaiRow*)malloc(need ? (size_t)need * sizeof(FaiRow) : 1);    // exactly the rows
        if (fai_events_host(d, n, by_rows.fed, c, rows, need, &tail) != need) { fprintf(stderr, "the second pass counts other rows\n"); return 1; }
        printf("window %u rows %lld\n", k, need);
        std::string hdr;                                                     // the header texts, as csv_fai_events_host lays them out
        const ref_i64 base = by_rows.fed;
        auto piece = [&](ref_i64 s, ref_i64 e) { const ref_i64 s0 = s < base ? base : s; if (e > s0) hdr.append((const char*)d + (s0 - base), (size_t)(e - s0)); };
        for (ref_i64 i = 0; i < need; i++) {
            printf("%lld %lld %lld\n", rows[i].start, rows[i].bytes, rows[i].bases);
            if (rows[i].bases & FAI_HDR) piece(rows[i].start, rows[i].start + rows[i].bytes);
        }
        if (tail.first == '>' && tail.start < base + n) piece(tail.start, base + n);
        char* h = (char*)malloc(hdr.size() ? hdr.size() : 1);                // exactly the header texts
        memcpy(h, hdr.data(), hdr.size());
        if (!by_rows.rows(rows, need, h, (ref_i64)hdr.size(), n, tail) && !by_rows.bad) rows_ok = false;   // (a refused text keeps counting its bytes)
        by_bytes.feed((const char*)d, n);
        free(h); free(rows); free(d);
    }
    if (!rows_ok) { fprintf(stderr, "the rows do not describe their window\n"); return 1; }
    print_index("rows", by_rows);
    print_index("bytes", by_bytes);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: ref_core_main CORPUS OUT | ref_core_main events WINDOWS\n"); return 2; }
    const bool ev = strcmp(argv[1], "events") == 0;
    FILE* fp = fopen(argv[ev ? 2 : 1], "rb");
    if (!fp) { perror(argv[ev ? 2 : 1]); return 2; }
    std::vector<unsigned char> f;
    unsigned char chunk[65536];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, fp)) > 0;) f.insert(f.end(), chunk, chunk + k);
    fclose(fp);
    if (ev) return events(f);
    size_t o = 0;
    const uint32_t nb = take<uint32_t>(f, o);
    std::vector<ref_i64> uoff(nb), data_off(nb);
    std::vector<int> isize(nb);
    std::vector<size_t> at(nb);
    size_t total = 0;
    for (uint32_t k = 0; k < nb; k++) {
        uoff[k] = take<int64_t>(f, o);
        isize[k] = (int)take<uint32_t>(f, o);
        at[k] = o; data_off[k] = (ref_i64)total;
        o += (size_t)isize[k]; total += (size_t)isize[k];
        if (o > f.size()) { fprintf(stderr, "the corpus is cut short\n"); return 2; }
    }
    uint8_t* data = (uint8_t*)malloc(total ? total : 1);                 // exactly the blocks' bytes
    for (uint32_t k = 0; k < nb; k++) memcpy(data + data_off[k], f.data() + at[k], (size_t)isize[k]);
    const RefBlocks B{(int)nb, uoff.data(), isize.data(), data_off.data(), data};
    const uint32_t nr = take<uint32_t>(f, o);
    std::vector<ref_i64> base_off(nr), beg(nr), end(nr), out_off(nr + 1, 0), tile_first(nr + 1, 0);
    std::vector<int> lb(nr), lw(nr), covered(nr);
    for (uint32_t r = 0; r < nr; r++) {
        base_off[r] = take<int64_t>(f, o); lb[r] = take<int32_t>(f, o); lw[r] = take<int32_t>(f, o); beg[r] = take<int64_t>(f, o); end[r] = take<int64_t>(f, o);
        covered[r] = ref_covered(B, base_off[r], lb[r], lw[r], beg[r], end[r]) ? 1 : 0;
        const ref_i64 n = covered[r] ? end[r] - beg[r] : 0;
        out_off[r + 1] = out_off[r] + n;
        tile_first[r + 1] = tile_first[r] + ref_tiles(n);
    }
    uint8_t* out = (uint8_t*)malloc(out_off[nr] ? (size_t)out_off[nr] : 1);      // exactly the ranges' bases
    const RefOneLane L;
    for (ref_i64 t = 0; t < tile_first[nr]; t++) ref_gather_tile(L, B, (ref_i64)nr, tile_first.data(), out_off.data(), base_off.data(), lb.data(), lw.data(), beg.data(), t, out);
    printf("tile %d\n", REF_TILE);
    for (uint32_t r = 0; r < nr; r++) printf("%u %d %lld\n", r, covered[r], out_off[r + 1] - out_off[r]);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    fwrite(out, 1, (size_t)out_off[nr], fo);
    fclose(fo);
    free(out);
    free(data);
    return 0;
}
