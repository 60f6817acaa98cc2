// index_core_main.cpp — cutesv_amd/csrc/index_core.h stand-alone, for the address and undefined-behaviour sanitizers
// (tests/test_index_build.py builds it with -fsanitize=address,undefined and the runtimes linked in; nothing is preloaded).
//   ix_reg2bin      against the loop of the specification (SAMv1 5.3), over the edge values of every level
//   ix_voff         over block tables with empty blocks, against a linear walk
//   ix::Builder     on random run sequences, fed record by record and as runs cut at random seams, against a naive dictionary form
// Prints "ok <checks>" and returns 0, or the first difference and 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "../cutesv_amd/csrc/index_core.h"

using namespace csv;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// the specification's own form
static int spec_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (int)(beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (int)(beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (int)(beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (int)(beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (int)(beg >> 26);
    return 0;
}

static long checks = 0;

static int check_reg2bin()
{
    std::vector<int64_t> pts = {0, 1, 2};
    for (int shift : {14, 17, 20, 23, 26, 29})
        for (int64_t k : {1, 2, 3})
            for (int64_t d : {-2, -1, 0, 1, 2}) { const int64_t v = (k << shift) + d; if (v >= 0 && v <= IX_MAX_POS) pts.push_back(v); }
    pts.push_back(IX_MAX_POS - 1); pts.push_back(IX_MAX_POS);
    for (int64_t b : pts)
        for (int64_t e : pts) {
            if (b >= e || b >= IX_MAX_POS) continue;
            const IxRec r = ix_record(b, e - b);
            checks++;
            if ((int)ix_reg2bin(b, e) != spec_reg2bin(b, e) || (int)r.bin != spec_reg2bin(b, e) || r.beg != b || r.end != e || r.w0 != (int32_t)(b >> 14) || r.w1 != (int32_t)((e - 1) >> 14)) {
                printf("reg2bin(%lld, %lld) = %u, the specification says %d\n", (long long)b, (long long)e, ix_reg2bin(b, e), spec_reg2bin(b, e));
                return 1;
            }
        }
    // pos < 0 and span 0: beg = 0, end >= 1
    const IxRec a = ix_record(-1, 0), z = ix_record(0, 0), far = ix_record(IX_MAX_POS, 5);
    if (a.beg != 0 || a.end != 1 || z.end != 1 || a.bin != 4681 || far.w1 != 0 || far.bin != 0) { printf("ix_record at the edges\n"); return 1; }
    const ix_i64 l_ref[2] = {100, 0};
    const IxCarry none{0, 0, 0, 0}, p5{1, 0, 50, 0}, tail{1, -1, -1, 0};
    const int got[] = {ix_refuse(2, 0, z, 2, l_ref, none), ix_refuse(-2, 0, z, 2, l_ref, none), ix_refuse(0, IX_MAX_POS, far, 2, l_ref, none), ix_refuse(0, 99, ix_record(99, 2), 2, l_ref, none),
                       ix_refuse(0, 99, ix_record(99, 1), 2, l_ref, none), ix_refuse(1, 0, z, 2, l_ref, none), ix_refuse(1, 0, ix_record(0, 2), 2, l_ref, none),
                       ix_refuse(0, 49, ix_record(49, 1), 2, l_ref, p5), ix_refuse(0, 50, ix_record(50, 1), 2, l_ref, p5), ix_refuse(1, 0, z, 2, l_ref, tail),
                       ix_refuse(-1, -1, ix_record(-1, 0), 2, l_ref, tail), ix_refuse(-1, -1, ix_record(-1, 0), 2, l_ref, p5)};
    const int want[] = {IX_E_REF, IX_E_REF, IX_E_RANGE, IX_E_REFLEN, IX_OK, IX_OK, IX_E_REFLEN, IX_E_ORDER, IX_OK, IX_E_ORDER, IX_OK, IX_OK};
    for (size_t k = 0; k < sizeof want / sizeof want[0]; k++) { checks++; if (got[k] != want[k]) { printf("ix_refuse case %zu: %d, expected %d\n", k, got[k], want[k]); return 1; } }
    if (ix_lin_entries(0) != 1 || ix_lin_entries(16383) != 1 || ix_lin_entries(16384) != 2 || ix_lin_entries(1ll << 31) != (1 << 15) + 1) { printf("ix_lin_entries\n"); return 1; }
    return 0;
}

static int check_voff()
{
    for (int round = 0; round < 200; round++) {
        const int n = 1 + (int)(rnd() % 12);
        std::vector<ix_i64> uoff, coff;
        std::vector<uint32_t> isize;
        ix_i64 u = 0, c = 0;
        for (int k = 0; k < n; k++) {
            const uint32_t len = (k == n - 1 || rnd() % 3 == 0) ? 0 : 1 + (uint32_t)(rnd() % 9);      // (the last block is the empty end-of-file block)
            uoff.push_back(u); coff.push_back(c); isize.push_back(len);
            u += len; c += 28 + (ix_i64)(rnd() % 50);
        }
        const IxBlocks B{uoff.data(), coff.data(), isize.data(), n};
        for (ix_i64 x = 0; x <= u; x++) {
            // the block that holds byte x: the first non-empty block whose range contains it; none: the last block, offset 0
            int k = 0;
            while (k < n - 1 && !(isize[(size_t)k] > 0 && x < uoff[(size_t)k] + (ix_i64)isize[(size_t)k])) k++;
            const ix_u64 want = ((ix_u64)coff[(size_t)k] << 16) | (ix_u64)(x - uoff[(size_t)k]);
            checks++;
            if (ix_voff(B, x) != want) { printf("ix_voff(%lld) = %llx, the walk says %llx (round %d)\n", (long long)x, ix_voff(B, x), want, round); return 1; }
        }
    }
    return 0;
}

// the naive form: per reference a dictionary bin -> chunks, a linear array grown on demand, counts; written as bai_writer.py writes
static std::vector<uint8_t> naive_bytes(int32_t n_ref, const std::vector<int32_t>& ref, const std::vector<IxRec>& rec, const std::vector<int>& unmapped,
                                        const std::vector<ix_u64>& vb, const std::vector<ix_u64>& ve)
{
    struct R { std::map<uint32_t, std::vector<std::pair<ix_u64, ix_u64>>> bins; std::vector<ix_u64> io; ix_u64 beg = 0, end = 0, m = 0, u = 0; bool any = false; };
    std::vector<R> refs((size_t)n_ref);
    ix_u64 nc = 0;
    for (size_t i = 0; i < ref.size(); i++) {
        if (ref[i] < 0) { nc++; continue; }
        R& x = refs[(size_t)ref[i]];
        (unmapped[i] ? x.u : x.m)++;
        if (!x.any) { x.any = true; x.beg = vb[i]; }
        x.end = ve[i];
        auto& ch = x.bins[rec[i].bin];
        if (!ch.empty() && ch.back().second == vb[i]) ch.back().second = ve[i]; else ch.emplace_back(vb[i], ve[i]);
        if ((size_t)rec[i].w1 + 1 > x.io.size()) x.io.resize((size_t)rec[i].w1 + 1, 0);
        for (int32_t w = rec[i].w0; w <= rec[i].w1; w++) if (x.io[(size_t)w] == 0 || vb[i] < x.io[(size_t)w]) x.io[(size_t)w] = vb[i];
    }
    std::vector<uint8_t> o = {'B', 'A', 'I', 1};
    auto p32 = [&](uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); };
    auto p64 = [&](ix_u64 v) { uint8_t b[8]; memcpy(b, &v, 8); o.insert(o.end(), b, b + 8); };
    p32((uint32_t)n_ref);
    for (R& x : refs) {
        for (size_t w = x.io.size(); w-- > 1;) if (x.io[w - 1] == 0) x.io[w - 1] = x.io[w];
        p32((uint32_t)x.bins.size() + (x.any ? 1u : 0u));
        for (auto& kv : x.bins) { p32(kv.first); p32((uint32_t)kv.second.size()); for (auto& c : kv.second) { p64(c.first); p64(c.second); } }
        if (x.any) { p32(IX_PSEUDO_BIN); p32(2); p64(x.beg); p64(x.end); p64(x.m); p64(x.u); }
        p32((uint32_t)x.io.size());
        for (ix_u64 v : x.io) p64(v);
    }
    p64(nc);
    return o;
}

static int check_builder()
{
    for (int round = 0; round < 300; round++) {
        const int32_t n_ref = 1 + (int32_t)(rnd() % 4);
        std::vector<ix_i64> l_ref;
        for (int32_t r = 0; r < n_ref; r++) l_ref.push_back(round % 7 == 0 ? 0 : 1 + (ix_i64)(rnd() % 400000));
        std::vector<int32_t> ref; std::vector<ix_i64> pos; std::vector<IxRec> rec; std::vector<int> unmapped; std::vector<ix_u64> vb, ve;
        ix_u64 v = 1000 + (rnd() % 50 << 16);
        for (int32_t r = 0; r < n_ref; r++) {
            if (rnd() % 4 == 0) continue;                                     // a reference without records
            ix_i64 p = 0;
            const int n = (int)(rnd() % 40);
            for (int k = 0; k < n; k++) {
                p += (ix_i64)(rnd() % (rnd() % 5 == 0 ? 30000 : 300));
                if (p >= l_ref[(size_t)r]) break;
                ix_i64 span = (ix_i64)(rnd() % (rnd() % 6 == 0 ? 100000 : 200));
                if (p + (span > 1 ? span : 1) > l_ref[(size_t)r]) span = l_ref[(size_t)r] - p;
                ref.push_back(r); pos.push_back(p); rec.push_back(ix_record(p, span)); unmapped.push_back(rnd() % 9 == 0);
                vb.push_back(v); v += (rnd() % 3 == 0) ? ((1 + rnd() % 3) << 16) : 40 + rnd() % 100; ve.push_back(v);
            }
        }
        for (int k = (int)(rnd() % 4); k > 0; k--) { ref.push_back(-1); pos.push_back(-1); rec.push_back(ix_record(-1, 0)); unmapped.push_back(1); vb.push_back(v); v += 50; ve.push_back(v); }
        const std::vector<uint8_t> want = naive_bytes(n_ref, ref, rec, unmapped, vb, ve);
        // (1) record by record, as the host routes feed it
        ix::Builder A;
        A.begin(n_ref, l_ref.data());
        for (size_t i = 0; i < ref.size(); i++) {
            if (ix_refuse(ref[i], pos[i], rec[i], n_ref, l_ref.data(), A.prev) != IX_OK) { printf("round %d: record %zu is refused\n", round, i); return 1; }
            A.add_record(ref[i], pos[i], rec[i], unmapped[i] != 0, vb[i], ve[i]);
        }
        // (2) as runs cut at random seams, with the arrays handed over whole, as the device route feeds it
        ix::Builder B;
        B.begin(n_ref, l_ref.data());
        B.lin = A.lin; B.counts = A.counts;
        IxRun cur{}; bool open = false;
        for (size_t i = 0; i < ref.size(); i++) {
            if (ref[i] < 0) break;
            const bool head = i == 0 || ref[i - 1] != ref[i] || rec[i - 1].bin != rec[i].bin, seam = rnd() % 5 == 0;
            if ((head || seam) && open) { B.add_run(cur); open = false; }
            if (!open) { cur = IxRun{vb[i], ve[i], ref[i], rec[i].bin, 0u, head ? 0u : 1u}; open = true; }
            cur.end = ve[i]; cur.n_records++;
        }
        if (open) B.add_run(cur);
        const std::vector<uint8_t> a = A.bytes(), b = B.bytes();
        checks += 2;
        if (a != want || b != want) { printf("round %d: the builder's bytes differ from the naive form (%zu, %zu, %zu bytes; records %s, runs %s)\n", round, a.size(), b.size(), want.size(), a == want ? "same" : "differ", b == want ? "same" : "differ"); return 1; }
        size_t n_rec = 0;
        for (const IxRun& r : B.runs) n_rec += r.n_records;
        size_t mapped = 0;
        for (int32_t r : ref) mapped += r >= 0;
        if (n_rec != mapped) { printf("round %d: the runs hold %zu records of %zu\n", round, n_rec, mapped); return 1; }
    }
    return 0;
}

int main()
{
    static_assert(sizeof(IxRun) == 32 && sizeof(IxVerdict) == 32 && sizeof(IxCarry) == 16, "the rows that cross the bus");
    if (check_reg2bin() || check_voff() || check_builder()) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
