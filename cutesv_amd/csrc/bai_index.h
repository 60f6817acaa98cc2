// bai_index.h — the BAM index (.bai) parser of the native reader.  Host C++ only, no dependency but the
// standard library: it compiles into libcutesv_hip.so beside bam_host.cpp and stand-alone (tests/bai_parse_main.cpp).
//
// Written from the SAM specification, section 5.2 "The BAI index format for BAM files":
//   magic "BAI\1", n_ref, then per reference
//     n_bin, { bin u32, n_chunk i32, { chunk_beg u64, chunk_end u64 } * n_chunk } * n_bin,
//     n_intv, { ioffset u64 } * n_intv                       (one per 16 384-base window: the smallest virtual offset of a
//                                                             record that overlaps the window)
//   and an optional n_no_coor u64 behind the last reference.  Bin 37450 is the pseudo-bin: two chunks, the second of which is
//   (n_mapped, n_unmapped).  A virtual offset is coffset << 16 | uoffset: the file offset of a BGZF block and a byte inside it.
//
// What is kept per reference is the linear index and the counts: bins and chunks are parsed and validated, then dropped.  The
// linear index alone gives a sound starting point for a region [beg, end): every record updates every window it overlaps, so
// whatever the level of its bin a record that overlaps `beg` lies at or behind ioffset[beg >> 14].
#ifndef CUTESV_BAI_INDEX_H
#define CUTESV_BAI_INDEX_H
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace bai {

constexpr int32_t  PSEUDO_BIN = 37450;
constexpr int32_t  MAX_BINS = 37451;           // bins 0 .. 37448 of the six levels, and the pseudo-bin
constexpr int32_t  MAX_INTV = 1 << 17;         // windows of 2^31 bases (the format indexes 2^29; l_ref is an int32)
constexpr int32_t  MAX_CHUNKS = 1 << 28;
constexpr int      WINDOW_SHIFT = 14;

struct Ref {
    std::vector<uint64_t> ioffset;             // the linear index, as in the file (0: no record overlaps the window)
    uint64_t n_mapped = 0, n_unmapped = 0;     // of the pseudo-bin; 0 without one
    bool     has_records = false;              // false: n_bin == 0 && n_intv == 0
};

struct Index {
    std::vector<Ref> refs;
    uint64_t n_no_coor = 0;
    bool     has_no_coor = false;
};

// 0: the virtual offset is fine; 1: its coffset is not the start of a block; 2: its uoffset is above the block's ISIZE
typedef int (*voff_check)(void* user, uint64_t voff);

namespace detail {
inline uint32_t u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline int32_t  i32(const uint8_t* p) { int32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t u64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

struct Cursor {
    const uint8_t* p; size_t n, at; const char* name; std::string* err;
    bool fail(const char* what, long long ref = -1, long long x = 0)
    {
        char buf[640];
        if (ref >= 0) snprintf(buf, sizeof buf, "%s: reference %lld: %s (%lld)", name, ref, what, x);
        else snprintf(buf, sizeof buf, "%s: %s (%lld)", name, what, x);
        *err = buf;
        return false;
    }
    bool need(size_t k, const char* field, long long ref)
    {
        if (n - at >= k) return true;
        char what[160];
        snprintf(what, sizeof what, "the file ends inside %s, at byte", field);
        return fail(what, ref, (long long)n);
    }
};

inline bool voff_ok(Cursor& c, voff_check check, void* user, uint64_t v, const char* field, long long ref)
{
    if (!check) return true;
    const int rc = check(user, v);
    if (rc == 0) return true;
    char what[200];
    snprintf(what, sizeof what, rc == 1 ? "%s: coffset %llu is not the start of a BGZF block of the BAM file; uoffset" : "%s: uoffset in the block at %llu is above its ISIZE:",
             field, (unsigned long long)(v >> 16));
    return c.fail(what, ref, (long long)(v & 0xffff));
}
}  // namespace detail

// data[0 .. n) is the whole index file; `name` is what the error texts call it; expect_n_ref < 0: not compared.
// -> true and *out, or false and *err (which names the file).  Nothing outside [data, data + n) is read.
inline bool parse(const uint8_t* data, size_t n, int32_t expect_n_ref, const char* name, voff_check check, void* user, Index* out, std::string* err)
{
    using namespace detail;
    Cursor c{data, n, 0, name, err};
    *out = Index();
    if (!c.need(4, "the magic", -1)) return false;
    if (memcmp(data, "BAI\1", 4) != 0) return c.fail("not a BAM index: no BAI\\1 magic at byte", -1, 0);
    c.at = 4;
    if (!c.need(4, "n_ref", -1)) return false;
    const int32_t n_ref = i32(data + c.at); c.at += 4;
    if (n_ref < 0) return c.fail("negative n_ref", -1, n_ref);
    if (expect_n_ref >= 0 && n_ref != expect_n_ref) {
        char what[160];
        snprintf(what, sizeof what, "the index has %d references, the BAM header has", n_ref);
        return c.fail(what, -1, expect_n_ref);
    }
    if ((size_t)n_ref > (n - c.at) / 8) return c.need(n - c.at + 1, "the references", -1);       // (each takes n_bin and n_intv at least)
    out->refs.resize((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; r++) {
        Ref& R = out->refs[(size_t)r];
        if (!c.need(4, "n_bin", r)) return false;
        const int32_t n_bin = i32(data + c.at); c.at += 4;
        if (n_bin < 0) return c.fail("negative n_bin", r, n_bin);
        if (n_bin > MAX_BINS) return c.fail("absurd n_bin", r, n_bin);
        for (int32_t k = 0; k < n_bin; k++) {
            if (!c.need(8, "a bin's header", r)) return false;
            const uint32_t bin = u32(data + c.at);
            const int32_t n_chunk = i32(data + c.at + 4); c.at += 8;
            if (n_chunk < 0) return c.fail("negative n_chunk", r, n_chunk);
            if (n_chunk > MAX_CHUNKS) return c.fail("absurd n_chunk", r, n_chunk);
            if (bin > (uint32_t)PSEUDO_BIN) return c.fail("bin number out of range", r, (long long)bin);
            if ((size_t)n_chunk > (n - c.at) / 16) return c.need(n - c.at + 1, "a bin's chunks", r);
            if (bin == (uint32_t)PSEUDO_BIN) {
                if (n_chunk != 2) return c.fail("the pseudo-bin 37450 needs two chunks, found", r, n_chunk);
                const uint64_t beg = u64(data + c.at), end = u64(data + c.at + 8);
                if (!voff_ok(c, check, user, beg, "pseudo-bin, first record", r) || !voff_ok(c, check, user, end, "pseudo-bin, end of the records", r)) return false;
                R.n_mapped = u64(data + c.at + 16); R.n_unmapped = u64(data + c.at + 24);
            } else {
                for (int32_t j = 0; j < n_chunk; j++) {
                    const uint64_t beg = u64(data + c.at + 16 * (size_t)j), end = u64(data + c.at + 16 * (size_t)j + 8);
                    if (end < beg) return c.fail("a chunk ends before it begins, bin", r, (long long)bin);
                    if (!voff_ok(c, check, user, beg, "chunk begin", r) || !voff_ok(c, check, user, end, "chunk end", r)) return false;
                }
            }
            c.at += 16 * (size_t)n_chunk;
        }
        if (!c.need(4, "n_intv", r)) return false;
        const int32_t n_intv = i32(data + c.at); c.at += 4;
        if (n_intv < 0) return c.fail("negative n_intv", r, n_intv);
        if (n_intv > MAX_INTV) return c.fail("absurd n_intv", r, n_intv);
        if ((size_t)n_intv > (n - c.at) / 8) return c.need(n - c.at + 1, "the linear index", r);
        R.ioffset.resize((size_t)n_intv);
        uint64_t last = 0;
        for (int32_t k = 0; k < n_intv; k++) {
            const uint64_t v = u64(data + c.at + 8 * (size_t)k);
            R.ioffset[(size_t)k] = v;
            if (v == 0) continue;                              // "no record overlaps this window"
            if (v < last) return c.fail("the linear index decreases at window", r, k);
            if (!voff_ok(c, check, user, v, "linear index", r)) return false;
            last = v;
        }
        c.at += 8 * (size_t)n_intv;
        R.has_records = n_bin != 0 || n_intv != 0;
    }
    if (c.at == n) return true;                               // no n_no_coor: it is optional
    if (!c.need(8, "n_no_coor", -1)) return false;
    out->n_no_coor = u64(data + c.at);
    out->has_no_coor = true;
    return true;
}

// Where a scan for records of reference `ref` that overlap a region beginning at `beg` may start: the entry of beg's window,
// or of the next window that has one.  -> false: no record of the reference overlaps any window from beg's on (an empty
// reference, a window at or behind n_intv, zeros to the end) - nothing needs to be read.
inline bool start_offset(const Index& ix, int32_t ref, int64_t beg, uint64_t* voff)
{
    if (ref < 0 || (size_t)ref >= ix.refs.size()) return false;
    const std::vector<uint64_t>& io = ix.refs[(size_t)ref].ioffset;
    const int64_t w = (beg < 0 ? 0 : beg) >> WINDOW_SHIFT;
    for (size_t k = (size_t)w; k < io.size(); k++)
        if (io[k]) { *voff = io[k]; return true; }
    return false;
}

// A guess at where the scan of a region that ends at `end` stops: the first entry of a window wholly at or behind `end`, in this
// reference or the next one that has any.  Only a guess (a long record may hold that window's entry far in front): it sizes
// what is inflated ahead, never what is read.  -> false: no later entry, the records end with the file.
inline bool stop_guess(const Index& ix, int32_t ref, int64_t end, uint64_t* voff)
{
    if (ref < 0 || (size_t)ref >= ix.refs.size()) return false;
    int64_t w = end <= 0 ? 0 : ((end - 1) >> WINDOW_SHIFT) + 1;
    for (size_t r = (size_t)ref; r < ix.refs.size(); r++, w = 0) {
        const std::vector<uint64_t>& io = ix.refs[r].ioffset;
        for (size_t k = (size_t)w; k < io.size(); k++)
            if (io[k]) { *voff = io[k]; return true; }
    }
    return false;
}

}  // namespace bai
#endif
