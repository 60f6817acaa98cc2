// csi_core_main.cpp — the CSI parser (cutesv_amd/csrc/csi_index.h) and ix::Builder::bytes_csi (index_core.h) as a stand-alone program:
// tests/test_csi_index.py builds it with -fsanitize=address,undefined and compares what it prints with what the library says of the
// same payloads.  Every payload, and every truncation of it, lives in a heap block of exactly its size, so a byte read behind a
// payload that ends inside a field is the sanitizer's to find.
//
//   csi_core_main CORPUS N_REF      CORPUS: u32 count, then per payload u32 bytes and the bytes; N_REF: the BAM header's n_ref
//   prints per payload:             index ok min_shift depth sum(table entries) sum(n_mapped) sum(n_unmapped) n_no_coor(-1: absent) start0 start_far
//                                   start0 / start_far: the lookup's virtual offset for reference 0 at position 0 / 2^29 (0: none)
//   then, for random builds under four schemes, fed record by record: bytes_csi() parses, equals the bytes of the same builder with
//   the per-bin loffsets handed in (the device route's form), and every truncation of it parses or is refused in bounds
//   last line:                      ok <checks>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cutesv_amd/csrc/csi_index.h"
#include "../cutesv_amd/csrc/index_core.h"

using namespace csv;

static long long checks = 0;

// parse data[0 .. n) out of a heap block of exactly n bytes
static bool parse_exact(const uint8_t* src, size_t n, int32_t n_ref, csi::Index* ix, std::string* err)
{
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(data, src, n);
    const bool ok = csi::parse(data, n, n_ref, "corpus.csi", nullptr, nullptr, ix, err);
    free(data);
    checks++;
    if (!ok && err->find("corpus.csi") == std::string::npos) { fprintf(stderr, "the error text does not name the file: %s\n", err->c_str()); exit(1); }
    return ok;
}

static void every_truncation(const std::vector<uint8_t>& p, int32_t n_ref)
{
    for (size_t n = 0; n < p.size(); n++) {
        csi::Index ix;
        std::string err;
        const bool ok = parse_exact(p.data(), n, n_ref, &ix, &err);
        uint64_t v;
        if (ok) for (size_t r = 0; r < ix.refs.size(); r++) { csi::start_offset(ix, (int32_t)r, 12345, &v); csi::stop_guess(ix, (int32_t)r, 1 << 20, &v); }
    }
}

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

static int builds()
{
    const int schemes[4][2] = {{14, 5}, {14, 6}, {12, 6}, {5, 2}};
    for (int round = 0; round < 40; round++) {
        const IxFormat F = ix_format(schemes[round % 4][0], schemes[round % 4][1]);
        const int32_t n_ref = 1 + (int32_t)(rnd() % 4);
        std::vector<ix_i64> l_ref;
        for (int32_t r = 0; r < n_ref; r++) l_ref.push_back(round % 9 == 0 ? 0 : 1 + (ix_i64)(rnd() % (uint64_t)(F.max_pos < 700000000 ? F.max_pos : 700000000)));
        ix::Builder A;
        A.begin(n_ref, l_ref.data(), F, true);
        ix_u64 v = 1000 + (rnd() % 50 << 16);
        for (int32_t r = 0; r < n_ref; r++) {
            if (rnd() % 4 == 0) continue;                        // an empty reference
            ix_i64 p = l_ref[(size_t)r] ? (ix_i64)(rnd() % (uint64_t)l_ref[(size_t)r]) : 0;
            for (int k = (int)(rnd() % 40); k > 0; k--) {
                p += (ix_i64)(rnd() % (rnd() % 5 == 0 ? (uint64_t)(F.max_pos / 64 + 1) : 300));
                ix_i64 span = (ix_i64)(rnd() % (rnd() % 6 == 0 ? (uint64_t)(F.max_pos / 16 + 1) : 200));
                const IxRec x = ix_record(p, span, F);
                if (ix_refuse(r, p, x, n_ref, l_ref.data(), A.prev, F) != IX_OK) break;
                A.add_record(r, p, x, rnd() % 9 == 0, v, v + 40);
                v += 40 + (rnd() % 7 == 0 ? (ix_u64)1 << 16 : 0);
            }
        }
        for (int k = (int)(rnd() % 3); k > 0; k--) { A.add_record(-1, -1, ix_record(-1, 0, F), true, v, v + 40); v += 40; }
        const std::vector<uint8_t> bytes = A.bytes_csi();
        csi::Index ix;
        std::string err;
        if (!parse_exact(bytes.data(), bytes.size(), n_ref, &ix, &err)) { printf("round %d: the built payload is refused: %s\n", round, err.c_str()); return 1; }
        if (ix.min_shift != F.min_shift || ix.depth != F.depth || !ix.has_no_coor) { printf("round %d: the header of the built payload\n", round); return 1; }
        // the device route's form: one loffset per pair, the first touched entry from the bin's first window on
        ix::Builder B = A;
        const std::vector<uint32_t> pairs = A.pairs();
        for (size_t k = 0; k < pairs.size() / 2; k++) {
            const ix_u64* io = A.lin.data() + A.lin_off[pairs[2 * k]];
            const ix_i64 n = A.lin_off[pairs[2 * k] + 1] - A.lin_off[pairs[2 * k]];
            ix_u64 found = IX_NONE;
            for (ix_i64 w = ix_bin_bot(pairs[2 * k + 1], F); w < n && found == IX_NONE; w++) found = io[w];
            if (found == IX_NONE) { printf("round %d: bin %u holds records and no window from its first one on is touched\n", round, pairs[2 * k + 1]); return 1; }
            B.loff.push_back(found);
        }
        B.has_loff = true;
        std::fill(B.lin.begin(), B.lin.end(), IX_NONE);
        checks++;
        if (B.bytes_csi() != bytes) { printf("round %d: the bytes from per-bin loffsets differ\n", round); return 1; }
        if (bytes.size() < 3000) every_truncation(bytes, n_ref);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: csi_core_main CORPUS N_REF\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int32_t n_ref = (int32_t)atoi(argv[2]);
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) { fprintf(stderr, "short corpus\n"); return 2; }
    for (uint32_t i = 0; i < count; i++) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1) { fprintf(stderr, "short corpus\n"); return 2; }
        std::vector<uint8_t> data(n);
        if (n && fread(data.data(), 1, n, f) != n) { fprintf(stderr, "short corpus\n"); return 2; }
        csi::Index ix;
        std::string err;
        if (!parse_exact(data.data(), n, n_ref, &ix, &err)) { printf("%u 0 0 0 0 0 0 0 0 0\n", i); continue; }
        unsigned long long entries = 0, mapped = 0, unmapped = 0;
        for (const csi::Ref& r : ix.refs) { entries += r.table.size(); mapped += r.n_mapped; unmapped += r.n_unmapped; }
        uint64_t v0 = 0, v1 = 0;
        if (!csi::start_offset(ix, 0, 0, &v0)) v0 = 0;
        if (!csi::start_offset(ix, 0, 1ll << 29, &v1)) v1 = 0;
        printf("%u 1 %d %d %llu %llu %llu %lld %llu %llu\n", i, ix.min_shift, ix.depth, entries, mapped, unmapped, ix.has_no_coor ? (long long)ix.n_no_coor : -1LL,
               (unsigned long long)v0, (unsigned long long)v1);
        if (n < 6000) every_truncation(data, n_ref);
    }
    fclose(f);
    if (builds()) return 1;
    printf("ok %lld\n", checks);
    return 0;
}
