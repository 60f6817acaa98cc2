// csi_index.h — the coordinate-sorted index (.csi) parser of the native reader.  Host C++ only, no dependency
// but the standard library and bai_index.h, whose cursor and virtual-offset check it shares: it compiles into libcutesv_hip.so beside
// bam_host.cpp and stand-alone (tests/csi_core_main.cpp).
//
// The format, as htslib writes it with `samtools index -c`.  The file is BGZF-compressed as a whole; parse() takes the inflated
// payload, little endian:
//   magic "CSI\1", min_shift i32, depth i32, l_aux i32, aux u8[l_aux], n_ref i32, then per reference
//     n_bin, { bin u32, loffset u64, n_chunk i32, { chunk_beg u64, chunk_end u64 } * n_chunk } * n_bin
//   and an optional n_no_coor u64 behind the last reference.
// Level 0 is the root; a bin of level l spans 2^(min_shift + 3 * (depth - l)) bases and the first bin of level l has the number
// ((1 << 3 * l) - 1) / 7.  With min_shift 14 and depth 5 the bins are BAI's.  The regular bins are 0 .. n_bins - 1 with
// n_bins = ((1 << 3 * (depth + 1)) - 1) / 7; the pseudo-bin is n_bins + 1 (37450 at depth 5): two chunks, the second of which is
// (n_mapped, n_unmapped), loffset 0.  There is no linear index: loffset(bin) is the entry a linear index of 2^min_shift-base windows,
// empty windows filled from the next touched one, has at the bin's first base - for a bin that holds records, the virtual offset of the
// first record in file order that overlaps the bin.
//
// What is kept per reference is the counts and a table (first base of a bin, loffset), sorted by base.  The filled linear index is
// monotone and every loffset is one of its values, so every record that overlaps `beg` or lies behind it is at or behind the loffset
// of the greatest table entry with base <= beg: a sound starting point, coarser than a .bai's wherever the bin of the deepest level
// at `beg` is not in the file.
#ifndef CUTESV_CSI_INDEX_H
#define CUTESV_CSI_INDEX_H
#include <algorithm>
#include <utility>

#include "bai_index.h"

namespace csi {

constexpr int32_t MAX_DEPTH = 10;              // bin numbers are 32 bits wide: ((1 << 33) - 1) / 7 still fits
constexpr int32_t MAX_CHUNKS = 1 << 28;

struct Ref {
    std::vector<std::pair<int64_t, uint64_t>> table;   // (first base of a bin, loffset), ascending in both
    uint64_t n_mapped = 0, n_unmapped = 0;     // of the pseudo-bin; 0 without one
    uint64_t first = 0;                        // the reference's first record: the pseudo-bin's first chunk, else the smallest chunk_beg
    bool     has_records = false;              // false: n_bin == 0
};

struct Index {
    int32_t  min_shift = 14, depth = 5;
    std::vector<Ref> refs;
    uint64_t n_no_coor = 0;
    bool     has_no_coor = false;
};

inline uint32_t level_first(int l) { return (uint32_t)((((uint64_t)1 << (3 * l)) - 1) / 7); }

// does an inflated payload begin like a .csi?
inline bool is_csi(const uint8_t* data, size_t n) { return n >= 4 && memcmp(data, "CSI\1", 4) == 0; }

// data[0 .. n) is the inflated payload of the index file; `name` is what the error texts call it; expect_n_ref < 0: not compared.
// -> true and *out, or false and *err (which names the file).  Nothing outside [data, data + n) is read.
inline bool parse(const uint8_t* data, size_t n, int32_t expect_n_ref, const char* name, bai::voff_check check, void* user, Index* out, std::string* err)
{
    using namespace bai::detail;
    Cursor c{data, n, 0, name, err};
    *out = Index();
    if (!c.need(4, "the magic", -1)) return false;
    if (!is_csi(data, n)) return c.fail("not a CSI index: no CSI\\1 magic at byte", -1, 0);
    c.at = 4;
    if (!c.need(12, "min_shift, depth and l_aux", -1)) return false;
    const int32_t min_shift = i32(data + 4), depth = i32(data + 8), l_aux = i32(data + 12);
    c.at = 16;
    if (min_shift < 1) return c.fail("min_shift below 1", -1, min_shift);
    if (depth < 0) return c.fail("negative depth", -1, depth);
    if (depth > MAX_DEPTH || min_shift > 62 || min_shift + 3 * depth > 62) return c.fail("min_shift + 3 * depth above 62 (or a depth whose bins do not fit 32 bits): min_shift", -1, min_shift);
    if (l_aux < 0) return c.fail("negative l_aux", -1, l_aux);
    if ((size_t)l_aux > n - c.at) return c.need(n - c.at + 1, "the aux data", -1);
    c.at += (size_t)l_aux;
    if (!c.need(4, "n_ref", -1)) return false;
    const int32_t n_ref = i32(data + c.at); c.at += 4;
    if (n_ref < 0) return c.fail("negative n_ref", -1, n_ref);
    if (expect_n_ref >= 0 && n_ref != expect_n_ref) {
        char what[160];
        snprintf(what, sizeof what, "the index has %d references, the BAM header has", n_ref);
        return c.fail(what, -1, expect_n_ref);
    }
    if ((size_t)n_ref > (n - c.at) / 4) return c.need(n - c.at + 1, "the references", -1);       // (each takes n_bin at least)
    out->min_shift = min_shift; out->depth = depth;
    const uint32_t n_bins = level_first(depth + 1), pseudo = n_bins + 1;
    char pseudo_what[96];
    snprintf(pseudo_what, sizeof pseudo_what, "the pseudo-bin %u needs two chunks, found", pseudo);
    out->refs.resize((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; r++) {
        Ref& R = out->refs[(size_t)r];
        if (!c.need(4, "n_bin", r)) return false;
        const int32_t n_bin = i32(data + c.at); c.at += 4;
        if (n_bin < 0) return c.fail("negative n_bin", r, n_bin);
        if ((uint32_t)n_bin > pseudo) return c.fail("absurd n_bin", r, n_bin);
        bool has_pseudo = false, any_chunk = false;
        uint64_t least = 0;
        for (int32_t k = 0; k < n_bin; k++) {
            if (!c.need(16, "a bin's header", r)) return false;
            const uint32_t bin = u32(data + c.at);
            const uint64_t loffset = u64(data + c.at + 4);
            const int32_t n_chunk = i32(data + c.at + 12); c.at += 16;
            if (n_chunk < 0) return c.fail("negative n_chunk", r, n_chunk);
            if (n_chunk > MAX_CHUNKS) return c.fail("absurd n_chunk", r, n_chunk);
            if (bin > pseudo) return c.fail("bin number out of range", r, (long long)bin);
            if ((size_t)n_chunk > (n - c.at) / 16) return c.need(n - c.at + 1, "a bin's chunks", r);
            if (bin == pseudo) {
                if (n_chunk != 2) return c.fail(pseudo_what, r, n_chunk);
                const uint64_t beg = u64(data + c.at), end = u64(data + c.at + 8);
                if (!voff_ok(c, check, user, beg, "pseudo-bin, first record", r) || !voff_ok(c, check, user, end, "pseudo-bin, end of the records", r)) return false;
                R.n_mapped = u64(data + c.at + 16); R.n_unmapped = u64(data + c.at + 24);
                R.first = beg; has_pseudo = true;
            } else {
                if (loffset && !voff_ok(c, check, user, loffset, "loffset", r)) return false;
                for (int32_t j = 0; j < n_chunk; j++) {
                    const uint64_t beg = u64(data + c.at + 16 * (size_t)j), end = u64(data + c.at + 16 * (size_t)j + 8);
                    if (end < beg) return c.fail("a chunk ends before it begins, bin", r, (long long)bin);
                    if (!voff_ok(c, check, user, beg, "chunk begin", r) || !voff_ok(c, check, user, end, "chunk end", r)) return false;
                    if (loffset > beg) return c.fail("the loffset lies behind a chunk of its own bin, bin", r, (long long)bin);
                    if (!any_chunk || beg < least) { least = beg; any_chunk = true; }
                }
                if (loffset && bin < n_bins) {                  // (bin n_bins itself is no bin of the scheme: nothing is kept of it)
                    int l = 0;
                    while (l < depth && bin >= level_first(l + 1)) l++;
                    const int64_t base = (int64_t)(((uint64_t)(bin - level_first(l)) << (3 * (depth - l))) << min_shift);
                    R.table.emplace_back(base, loffset);
                }
            }
            c.at += 16 * (size_t)n_chunk;
        }
        if (!has_pseudo) R.first = least;
        R.has_records = n_bin != 0;
        // by base, the minimum per base; in a sorted file the loffset cannot decrease with the base
        std::sort(R.table.begin(), R.table.end());
        size_t m = 0;
        for (size_t k = 0; k < R.table.size(); k++)
            if (m == 0 || R.table[k].first != R.table[m - 1].first) R.table[m++] = R.table[k];
        R.table.resize(m);
        for (size_t k = 1; k < m; k++)
            if (R.table[k].second < R.table[k - 1].second) return c.fail("the loffset decreases at base", r, (long long)R.table[k].first);
    }
    if (c.at == n) return true;                               // no n_no_coor: it is optional
    if (!c.need(8, "n_no_coor", -1)) return false;
    out->n_no_coor = u64(data + c.at);
    out->has_no_coor = true;
    return true;
}

// Where a scan for records of reference `ref` that overlap a region beginning at `beg` may start: the loffset of the greatest table
// entry with base <= beg; without one, the reference's first record.  -> false: the reference has no bins, hence no records -
// nothing needs to be read.
inline bool start_offset(const Index& ix, int32_t ref, int64_t beg, uint64_t* voff)
{
    if (ref < 0 || (size_t)ref >= ix.refs.size()) return false;
    const Ref& R = ix.refs[(size_t)ref];
    if (!R.has_records) return false;
    if (beg < 0) beg = 0;
    auto it = std::upper_bound(R.table.begin(), R.table.end(), std::make_pair(beg, ~(uint64_t)0));
    *voff = it == R.table.begin() ? R.first : (it - 1)->second;
    return true;
}

// A guess at where the scan of a region that ends at `end` stops: the first table entry with base >= end, else the first record of
// the next reference that has any.  Only a guess: it sizes what is inflated ahead, never what is read.  -> false: no later entry.
inline bool stop_guess(const Index& ix, int32_t ref, int64_t end, uint64_t* voff)
{
    if (ref < 0 || (size_t)ref >= ix.refs.size()) return false;
    const Ref& R = ix.refs[(size_t)ref];
    auto it = std::lower_bound(R.table.begin(), R.table.end(), std::make_pair(end, (uint64_t)0));
    if (it != R.table.end()) { *voff = it->second; return true; }
    for (size_t r = (size_t)ref + 1; r < ix.refs.size(); r++)
        if (ix.refs[r].has_records && ix.refs[r].first) { *voff = ix.refs[r].first; return true; }
    return false;
}

}  // namespace csi
#endif
