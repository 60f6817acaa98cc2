// bai_parse_main.cpp — the BAM index parser (cutesv_amd/csrc/bai_index.h) over a corpus of index files, as a stand-alone program:
// tests/test_bam_index.py builds it with -fsanitize=address,undefined and compares what it prints with what the library says of
// the same files.  Every index lives in a heap block of exactly its size, so a byte read behind a file that ends inside a field is
// the sanitizer's to find.
//
//   bai_parse_main CORPUS N_REF     CORPUS: u32 count, then per index u32 bytes and the bytes; N_REF: the BAM header's n_ref
//   prints per index:               index ok n_ref sum(n_intv) sum(n_mapped) sum(n_unmapped) n_no_coor(-1: absent) start0   (ok = 0: zeros)
//                                   start0: the lookup's virtual offset for reference 0, position 0 (0: none)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cutesv_amd/csrc/bai_index.h"

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: bai_parse_main CORPUS N_REF\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int32_t n_ref = (int32_t)atoi(argv[2]);
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) { fprintf(stderr, "short corpus\n"); return 2; }
    for (uint32_t i = 0; i < count; i++) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) { fprintf(stderr, "short corpus\n"); return 2; }
        uint8_t* data = (uint8_t*)malloc(n ? n : 1);          // exactly the file's size (1 for an empty file: malloc(0) may be NULL)
        if (n && fread(data, 1, n, f) != n) { fprintf(stderr, "short corpus\n"); return 2; }
        bai::Index ix;
        std::string err;
        const bool ok = bai::parse(data, n, n_ref, "corpus.bai", nullptr, nullptr, &ix, &err);
        free(data);
        if (!ok) {
            if (err.find("corpus.bai") == std::string::npos) { fprintf(stderr, "index %u: the error text does not name the file: %s\n", i, err.c_str()); return 1; }
            printf("%u 0 0 0 0 0 0 0\n", i);
            continue;
        }
        unsigned long long intv = 0, mapped = 0, unmapped = 0;
        for (const bai::Ref& r : ix.refs) { intv += r.ioffset.size(); mapped += r.n_mapped; unmapped += r.n_unmapped; }
        uint64_t v = 0;
        if (!bai::start_offset(ix, 0, 0, &v)) v = 0;
        printf("%u 1 %zu %llu %llu %llu %lld %llu\n", i, ix.refs.size(), intv, mapped, unmapped, ix.has_no_coor ? (long long)ix.n_no_coor : -1LL, (unsigned long long)v);
    }
    fclose(f);
    return 0;
}
