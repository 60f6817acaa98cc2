// sort_core.h — coordinate-sorting a BAM's records, written once for the host and for the device.  Plain
// C++: no HIP header, no global state.  Four rules live here, and nowhere else:
//   the key       sort_key: one uint64 per record out of its bytes, refid' << 33 | (pos + 1) << 1 | reverse-strand bit, with
//                 refid' = n_ref for refid -1 (records without a reference sort last) and pos -1 first on its contig.  Records of equal
//                 key keep their input order: every user of the key sorts stably.  The order restates samtools' coordinate order
//                 from memory; the tests judge it against an independent stable sort, never against samtools.
//   the refusal   sort_refuse / sort_refusal_text: a refid outside [-1, n_ref) or a pos below -1 has no place in that order.
//   the tile      The sorted stream is the rewritten header (H bytes) and behind it the records in sorted order; dst[i] is the
//                 exclusive prefix sum of 4 + block_size over the sorted records (dst[n]: their total).  sort_first_record finds by
//                 binary search the record that holds a byte of the record area; sort_tile_fill writes any byte range [t0, t1) of the
//                 stream as the concatenation of header and record pieces.  The device's gather (k_sort_gather, at the end of bam.hip.h) uses the same
//                 search and the same piece rule, 16 bytes per lane.
//   the header    sort_header: the BAM header with @HD's SO: set to coordinate (host only).
// tests/sort_core_main.cpp runs all of it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SORT_FN __host__ __device__ inline
#else
#define SORT_FN inline
#endif

namespace csv {

typedef long long so_i64;
typedef unsigned long long so_u64;

constexpr so_u64 SORT_NONE = ~0ull;                   // the verdict word when no record is refused (ordinal << 3 | why otherwise)
constexpr int SORT_WHY_REFID = 1, SORT_WHY_POS = 2, SORT_WHY_CHAIN = 3;      // (CHAIN: the device's own guard, never a property of a file)
constexpr so_i64 SORT_BLOCK = 65280;                  // bytes of the sorted stream per BGZF block (bgzip's cut, deflate_core.h's DFL_MAX_IN)
constexpr int SORT_SLICE_BLOCKS = 256;                // blocks per slice when the caller names none (16 MiB of stream)

SORT_FN uint32_t so_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the fields of the key, from the record's first byte (its block_size word): refid at + 4, pos at + 8, flag at + 18.  The caller
// knows that [p, p + 36) is readable: the reader stepped over the record, whose block_size is 32 or more
struct SortFields { int32_t refid, pos; uint32_t flag; so_i64 len; };
SORT_FN SortFields sort_fields(const uint8_t* p)
{
    SortFields f;
    f.len = 4 + (so_i64)(int32_t)so_u32(p);
    f.refid = (int32_t)so_u32(p + 4); f.pos = (int32_t)so_u32(p + 8);
    f.flag = (uint32_t)p[18] | ((uint32_t)p[19] << 8);
    return f;
}

// 0: the record has a place in the order; else why not
SORT_FN int sort_refuse(const SortFields& f, int32_t n_ref)
{
    if (f.refid < -1 || f.refid >= n_ref) return SORT_WHY_REFID;
    if (f.pos < -1) return SORT_WHY_POS;
    return 0;
}

// the key of a record that sort_refuse accepts
SORT_FN so_u64 sort_key(const SortFields& f, int32_t n_ref)
{
    const so_u64 r = f.refid < 0 ? (so_u64)(uint32_t)n_ref : (so_u64)(uint32_t)f.refid;
    return r << 33 | (so_u64)((so_i64)f.pos + 1) << 1 | (so_u64)((f.flag >> 4) & 1u);
}

// the largest key a file of n_ref references can hold, whatever its records say, and every bit a key below it can have set: which
// 8-bit digits a radix sort may have to look at
SORT_FN so_u64 sort_key_bound(int32_t n_ref) { return (so_u64)(uint32_t)n_ref << 33 | 0x1ffffffffull; }
SORT_FN so_u64 sort_key_bits(int32_t n_ref)
{
    so_u64 m = sort_key_bound(n_ref);
    for (int s = 1; s < 64; s <<= 1) m |= m >> s;
    return m;
}

// the largest i in [lo, hi] with dst[i] <= x; the caller knows dst[lo] <= x.  dst is strictly increasing (a record has 36 bytes or more)
SORT_FN so_i64 sort_first_record(const so_i64* dst, so_i64 lo, so_i64 hi, so_i64 x)
{
    while (lo < hi) {
        const so_i64 m = lo + (hi - lo + 1) / 2;
        if (dst[m] <= x) lo = m; else hi = m - 1;
    }
    return lo;
}

// bytes [t0, t1) of the sorted stream into out[0 .. t1 - t0): header bytes, then pieces of the records perm[r] (perm NULL: the
// identity), found from the first record that feeds the tile on.  0 <= t0 <= t1 <= H + dst[n]
SORT_FN void sort_tile_fill(uint8_t* out, so_i64 t0, so_i64 t1, const uint8_t* hdr, so_i64 H, const uint8_t* arena, const so_i64* starts, const int32_t* perm, const so_i64* dst,
                            so_i64 n)
{
    so_i64 o = t0;
    for (; o < t1 && o < H; o++) out[o - t0] = hdr[o];
    if (o >= t1 || n <= 0) return;
    so_i64 r = sort_first_record(dst, 0, n - 1, o - H);
    while (o < t1) {
        const so_i64 in_rec = o - H - dst[r], left = dst[r + 1] - dst[r] - in_rec, want = t1 - o, k = left < want ? left : want;
        const uint8_t* src = arena + starts[perm ? perm[r] : r] + in_rec;
        for (so_i64 j = 0; j < k; j++) out[o - t0 + j] = src[j];
        o += k; r++;
    }
}

}  // namespace csv

#include <string>
#include <vector>

namespace csv {

// what a refused record is told, behind "cannot sort: record <ordinal> "; the same on every route
inline std::string sort_refusal_text(int why, int32_t n_ref)
{
    if (why == SORT_WHY_REFID) return "has a refID outside -1 .. " + std::to_string((long long)n_ref - 1) + ", the references of the header";
    return "has a pos below -1";
}

// The header rule.  head[0 .. n) is a BAM header: magic, l_text, text, n_ref and the reference list.  The copy differs in the text
// alone, in one place: the first @HD line gets SO:coordinate where its SO: field stood (appended when it had none) and loses any GO:
// or SS: field, which would contradict the new order; a text without an @HD line gets "@HD\tVN:1.6\tSO:coordinate\n" in front.  l_text
// follows; the reference list is copied as it is; no @PG line is added: the output is a pure function of the input.
// false: head is no BAM header
inline bool sort_header(const uint8_t* head, so_i64 n, std::vector<uint8_t>* out)
{
    if (n < 12 || memcmp(head, "BAM\1", 4) != 0) return false;
    const so_i64 l_text = (int32_t)so_u32(head + 4);
    if (l_text < 0 || 8 + l_text + 4 > n) return false;
    const std::string text((const char*)head + 8, (size_t)l_text);
    size_t at = 0, hd = std::string::npos, hd_end = 0;
    while (at < text.size() && text[at] != '\0') {                           // (NUL padding behind the text is no line)
        size_t e = text.find('\n', at);
        if (e == std::string::npos) e = text.size();
        if (text.compare(at, 3, "@HD") == 0 && (at + 3 == e || text[at + 3] == '\t')) { hd = at; hd_end = e; break; }
        at = e + 1;
    }
    std::string t;
    if (hd == std::string::npos) t = "@HD\tVN:1.6\tSO:coordinate\n" + text;
    else {
        std::string line = "@HD";
        bool placed = false;
        for (size_t f = hd + 3; f < hd_end;) {                               // the fields: each begins behind a tab
            size_t fe = text.find('\t', f + 1);
            if (fe == std::string::npos || fe > hd_end) fe = hd_end;
            const std::string field = text.substr(f + 1, fe - f - 1);
            if (field.compare(0, 3, "SO:") == 0) { if (!placed) line += "\tSO:coordinate"; placed = true; }
            else if (field.compare(0, 3, "GO:") != 0 && field.compare(0, 3, "SS:") != 0) line += "\t" + field;
            f = fe;
        }
        if (!placed) line += "\tSO:coordinate";
        t = text.substr(0, hd) + line + text.substr(hd_end);
    }
    out->clear();
    out->insert(out->end(), head, head + 4);
    const uint32_t lt = (uint32_t)t.size();
    for (int k = 0; k < 4; k++) out->push_back((uint8_t)(lt >> (8 * k)));
    out->insert(out->end(), t.begin(), t.end());
    out->insert(out->end(), head + 8 + l_text, head + n);
    return true;
}

}  // namespace csv

// ---- The sort's way to the device (stage_bam_sort.hip.h), for bam_host.cpp alone: inside the library, not part of the C ABI.
// csv_sort_begin: room for an arena of arena_bytes - the inflated stream, at its own offsets - and the header image.  csv_sort_append:
// bytes [arena_off, + len) arrive, from host memory (src) or, src NULL, from offset win_off of the context's framing window.
// csv_sort_order: the n record starts (arena offsets, chained and inside the arena: the reader stepped over every record) -> keys,
// verdict, permutation, dst.  csv_sort_slice: bytes [s0, s0 + len) of the sorted stream, len <= slice bytes, gathered and compressed
// in blocks of SORT_BLOCK bytes; only the blocks come down.  csv_sort_end: the arena is given back.
struct csv_ctx;
// Weak: a build of bam_host.cpp without the library's device side (tests/bam_host_main.cpp) links, and the sort says that it has no
// device route there.
#define SORT_LOCAL extern "C" __attribute__((visibility("hidden"), weak))
struct csv_sort_verdict { unsigned long long bad; long long inversions, record_bytes; int passes; };
SORT_LOCAL int csv_sort_free_bytes(csv_ctx* c, int64_t* free_bytes);
SORT_LOCAL int csv_sort_begin(csv_ctx* c, int64_t arena_bytes, const uint8_t* hdr, int64_t hdr_bytes, int64_t slice_bytes);
SORT_LOCAL int csv_sort_append(csv_ctx* c, int64_t arena_off, const uint8_t* src, int64_t win_off, int64_t len);
SORT_LOCAL int csv_sort_order(csv_ctx* c, int64_t n, const int64_t* starts, int32_t n_ref, csv_sort_verdict* v);
SORT_LOCAL int csv_sort_slice(csv_ctx* c, int64_t s0, int64_t len, uint8_t* out, int64_t out_cap, int32_t* block_bytes, int64_t* out_bytes);
SORT_LOCAL int csv_sort_counters(csv_ctx* c, double* ms4, int64_t* bytes_up, int64_t* bytes_down);
SORT_LOCAL int csv_sort_end(csv_ctx* c);
