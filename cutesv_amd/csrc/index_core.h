// index_core.h — building a BAM index (.bai, or .csi under a binning scheme of its own) from the records of a file, written once for
// the host and for the device (DESIGN.md sections 30 and 32).  Plain C++: no HIP header, no global state; the style of frame_core.h and inflate_core.h.
//
// The per-record rules (SAMv1 sections 5.2 and 5.3), for a record with refID >= 0:
//   beg = max(pos, 0), end = max(pos + max(span, 1), 1)     span: the sum over M / D / N / = / X of the record's own CIGAR words
//   bin = ix_reg2bin(beg, end); the linear-index windows it overlaps are [beg >> 14, (end - 1) >> 14]
//   its chunk is [ix_voff(start), ix_voff(start + 4 + block_size)) - virtual offsets, coffset << 16 | uoffset
// A RUN is a maximal stretch of neighbours in file order with one (refID, bin): it becomes one chunk of that bin.  ioffset[w] is
// the virtual offset of the first record in file order that overlaps window w - the minimum, as the file is sorted.
//   IxFormat                the binning scheme: BAI's {14, 5, 2^29} is the default argument everywhere, so the rules above are its case
//   ix_reg2bin, ix_record   the rules above
//   ix_refuse               what cannot be indexed (IX_E_*): the same predicates in the same order on every route
//   ix_voff                 a stream offset -> its virtual offset, by binary search over the whole-file block table
//   IxRun, IxVerdict        what comes down per window on the device route (k_index_rows, k_index_runs at the end of bam.hip.h)
//   ix::Builder             host only: runs in file order + the linear arrays + the counts -> the bytes of the index (bytes(): a .bai;
//                           bytes_csi(): the payload of a .csi).  Both routes end here; tests/index_core_main.cpp and
//                           tests/csi_core_main.cpp run it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INDEX_FN __host__ __device__ inline
#else
#define INDEX_FN inline
#endif

namespace csv {

typedef long long ix_i64;
typedef unsigned long long ix_u64;

constexpr ix_i64   IX_MAX_POS = 1ll << 29;         // the BAI format indexes [0, 2^29)
constexpr int      IX_WINDOW_SHIFT = 14;
constexpr uint32_t IX_PSEUDO_BIN = 37450;
constexpr ix_u64   IX_NONE = ~0ull;                // a linear-index entry no record has touched
constexpr int      IX_LANE_WINDOWS = 4;            // windows a record's own lane writes; the wavefront shares the rest (k_index_rows)

enum { IX_OK = 0, IX_E_REF = 1, IX_E_RANGE = 2, IX_E_REFLEN = 3, IX_E_ORDER = 4 };

// the binning scheme: 2^min_shift bases in a bin of the deepest level, `depth` levels under the root, [0, max_pos) indexed.  The BAI
// format is the scheme {14, 5, 2^29}; a CSI index (csi_index.h) carries its own
struct IxFormat { int32_t min_shift, depth; ix_i64 max_pos; };

INDEX_FN IxFormat ix_format(int32_t min_shift, int32_t depth) { return IxFormat{min_shift, depth, (ix_i64)1 << (min_shift + 3 * depth)}; }
INDEX_FN IxFormat ix_bai() { return IxFormat{IX_WINDOW_SHIFT, 5, IX_MAX_POS}; }
// what a build takes: windows of 16 bases at least (an int32 window number), bins in 32 bits, positions in 62
INDEX_FN bool ix_format_ok(const IxFormat& F) { return F.min_shift >= 4 && F.min_shift <= 31 && F.depth >= 0 && F.depth <= 9 && F.min_shift + 3 * F.depth <= 62; }
// the first bin of level l (0: the root), the regular bins of the scheme, its pseudo-bin, the first deepest-level window of a bin
INDEX_FN uint32_t ix_level_first(int l) { return (uint32_t)((((ix_u64)1 << (3 * l)) - 1) / 7); }
INDEX_FN uint32_t ix_n_bins(const IxFormat& F) { return ix_level_first(F.depth + 1); }
INDEX_FN uint32_t ix_pseudo_bin(const IxFormat& F) { return ix_n_bins(F) + 1; }
INDEX_FN ix_i64 ix_bin_bot(uint32_t bin, const IxFormat& F)
{
    int l = 0;
    while (l < F.depth && bin >= ix_level_first(l + 1)) l++;
    return (ix_i64)(bin - ix_level_first(l)) << (3 * (F.depth - l));
}

// the bin of [beg, end), 0 <= beg < end <= max_pos: the deepest bin that holds both beg and end - 1 (the UCSC scheme of
// specification 5.3 under BAI)
INDEX_FN uint32_t ix_reg2bin(ix_i64 beg, ix_i64 end, const IxFormat& F = ix_bai())
{
    --end;
    int s = F.min_shift;
    for (int l = F.depth; l > 0; l--, s += 3)
        if (beg >> s == end >> s) return ix_level_first(l) + (uint32_t)(beg >> s);
    return 0;
}

struct IxRec { ix_i64 beg, end; uint32_t bin; int32_t w0, w1; };

INDEX_FN IxRec ix_record(ix_i64 pos, ix_i64 span, const IxFormat& F = ix_bai())
{
    IxRec r;
    r.beg = pos > 0 ? pos : 0;
    r.end = pos + (span > 1 ? span : 1);
    if (r.end < 1) r.end = 1;
    r.bin = 0; r.w0 = 0; r.w1 = 0;
    if (r.beg < F.max_pos && r.end <= F.max_pos) {             // (outside: refused, nothing of it is used)
        r.bin = ix_reg2bin(r.beg, r.end, F);
        r.w0 = (int32_t)(r.beg >> F.min_shift); r.w1 = (int32_t)((r.end - 1) >> F.min_shift);
    }
    return r;
}

// entries of a reference's linear array: every window a record that passes ix_refuse can touch
INDEX_FN ix_i64 ix_lin_entries(ix_i64 l_ref, const IxFormat& F = ix_bai())
{
    if (l_ref < 0) l_ref = 0;
    return ((l_ref < F.max_pos ? l_ref : F.max_pos) >> F.min_shift) + 1;
}

// the predecessor of a record in file order, as the head flag and the order rule need it
struct IxCarry { int32_t valid, ref; int32_t pos; uint32_t bin; };

// IX_OK, or why the record cannot be indexed.  refID -1 sorts last; a record without coordinates is only held to the order.
INDEX_FN int ix_refuse(int32_t ref, ix_i64 pos, const IxRec& r, int32_t n_ref, const ix_i64* l_ref, const IxCarry& prev, const IxFormat& F = ix_bai())
{
    if (ref < -1 || ref >= n_ref) return IX_E_REF;
    if (ref >= 0) {
        if (r.beg >= F.max_pos || r.end > F.max_pos) return IX_E_RANGE;
        const ix_i64 l = l_ref[ref] > 1 ? l_ref[ref] : 1;
        if (r.end > l) return IX_E_REFLEN;
    }
    if (prev.valid) {
        if ((uint32_t)ref < (uint32_t)prev.ref) return IX_E_ORDER;
        if (ref == prev.ref && ref >= 0 && pos < (ix_i64)prev.pos) return IX_E_ORDER;
    }
    return IX_OK;
}

// (the BAI texts; under a CSI scheme IX_E_RANGE has its own: ix::refusal_text below)
INDEX_FN const char* ix_refusal_text(int code)
{
    switch (code) {
    case IX_E_REF:    return "has a reference id that the header does not have";
    case IX_E_RANGE:  return "reaches 2^29 bases or beyond, which the BAI format cannot index";
    case IX_E_REFLEN: return "ends beyond the length of its reference";
    case IX_E_ORDER:  return "is out of coordinate order against the record before it";
    default:          return "cannot be indexed";
    }
}

// the whole-file block table: block k holds the stream bytes [uoff[k], uoff[k] + isize[k]) and starts at file byte coff[k]
struct IxBlocks { const ix_i64* uoff; const ix_i64* coff; const uint32_t* isize; ix_i64 n; };

// the virtual offset of stream byte u (0 <= u <= the stream's length, n >= 1): taken in the block that holds u; an empty block holds
// no byte, so a byte on a block boundary belongs to the next non-empty block with offset 0 - and the end of the stream to the last
// block, the end-of-file block
INDEX_FN ix_u64 ix_voff(const IxBlocks& B, ix_i64 u)
{
    ix_i64 lo = 0, hi = B.n;
    while (hi - lo > 1) { const ix_i64 m = (lo + hi) / 2; if (B.uoff[m] <= u) lo = m; else hi = m; }
    while (lo + 1 < B.n && B.isize[lo] == 0) lo++;
    return ((ix_u64)B.coff[lo] << 16) | (ix_u64)(u - B.uoff[lo]);
}

// one run, as a window of the device route hands it down (32 bytes).  continues: the window's first record carried on the run
// of the record before it - beg / ref / bin are that record's own, the host joins the row to the run it has
struct IxRun { ix_u64 beg, end; int32_t ref; uint32_t bin; uint32_t n_records; uint32_t continues; };

// what else comes down per window (32 bytes).  bad: the smallest (ordinal << 3 | IX_E_*) of a record ix_refuse turns away, IX_NONE:
// none; n_runs: rows of IxRun; last: the window's last record, the next window's carry
struct IxVerdict { ix_u64 bad; ix_i64 n_runs; IxCarry last; };

}  // namespace csv

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace csv {
namespace ix {

// why a record cannot be indexed: the BAI texts, but for the range of a CSI build, which names its scheme
inline std::string refusal_text(int code, const IxFormat& F, bool csi)
{
    if (code != IX_E_RANGE || !csi) return ix_refusal_text(code);
    char buf[200];
    snprintf(buf, sizeof buf, "reaches 2^%d bases or beyond, which a CSI index with min_shift %d and depth %d cannot index", F.min_shift + 3 * F.depth, F.min_shift, F.depth);
    return buf;
}

// htslib's rule for the depth: the smallest with max(l_ref) + 256 <= 2^(min_shift + 3 * depth)
inline int32_t auto_depth(int32_t min_shift, int32_t n_ref, const ix_i64* l_ref)
{
    ix_i64 max_len = 0;
    for (int32_t r = 0; r < n_ref; r++) if (l_ref[r] > max_len) max_len = l_ref[r];
    max_len += 256;
    int32_t depth = 0;
    while (min_shift + 3 * depth < 62 && max_len > ((ix_i64)1 << (min_shift + 3 * depth))) depth++;
    return depth;
}

// The assembler.  Fed in file order: add_record (the host routes: every record) or add_run + the arrays (the device route: lin and
// counts are the device's, handed over whole).  bytes(): magic, n_ref, per reference {bins ascending, each with its chunks in file
// order; the pseudo-bin; the filled linear index}, n_no_coor - what samtools and htslib write, and tests/bai_writer.py.
struct Builder {
    int32_t n_ref = 0;
    std::vector<ix_i64> lin_off;               // n_ref + 1: where a reference's entries start in `lin`
    std::vector<ix_u64> lin;                   // IX_NONE: untouched
    std::vector<ix_u64> counts;                // mapped, unmapped per reference; then n_no_coor
    std::vector<IxRun>  runs;
    ix_i64              records = 0;
    IxCarry             prev{0, 0, 0, 0};
    IxFormat            fmt = ix_bai();
    bool                csi = false;           // the build is for bytes_csi(): the refusals name the scheme
    std::vector<ix_u64> loff;                  // the device route of a CSI build: one loffset per distinct (ref, bin) of `pairs()`, in
    bool                has_loff = false;      // ... that order, instead of `lin`, which then stays IX_NONE

    void begin(int32_t nref, const ix_i64* l_ref, const IxFormat& F = ix_bai(), bool for_csi = false)
    {
        n_ref = nref; records = 0; prev = IxCarry{0, 0, 0, 0}; fmt = F; csi = for_csi;
        loff.clear(); has_loff = false;
        lin_off.assign((size_t)nref + 1, 0);
        for (int32_t r = 0; r < nref; r++) lin_off[(size_t)r + 1] = lin_off[(size_t)r] + ix_lin_entries(l_ref[r], F);
        lin.assign((size_t)lin_off[(size_t)nref], IX_NONE);
        counts.assign(2 * (size_t)nref + 1, 0);
        runs.clear();
    }

    // a run in file order; a `continues` row lengthens the run before it
    void add_run(const IxRun& r)
    {
        if (r.ref < 0 || r.ref >= n_ref) return;
        if (r.continues && !runs.empty()) { runs.back().end = r.end; runs.back().n_records += r.n_records; return; }
        runs.push_back(r);
        runs.back().continues = 0;
    }

    // one record that passed ix_refuse, with its two virtual offsets
    void add_record(int32_t ref, ix_i64 pos, const IxRec& r, bool unmapped_flag, ix_u64 vbeg, ix_u64 vend)
    {
        records++;
        if (ref < 0) { counts[2 * (size_t)n_ref]++; prev = IxCarry{1, ref, (int32_t)pos, 0}; return; }
        counts[2 * (size_t)ref + (unmapped_flag ? 1 : 0)]++;
        const bool head = !prev.valid || prev.ref != ref || prev.bin != r.bin;
        add_run(IxRun{vbeg, vend, ref, r.bin, 1u, head ? 0u : 1u});
        ix_u64* io = lin.data() + lin_off[(size_t)ref];
        for (int32_t w = r.w0; w <= r.w1; w++) if (vbeg < io[w]) io[w] = vbeg;
        prev = IxCarry{1, ref, (int32_t)pos, r.bin};
    }

    static void put32(std::vector<uint8_t>& o, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); o.insert(o.end(), b, b + 4); }
    static void put64(std::vector<uint8_t>& o, ix_u64 v) { uint8_t b[8]; memcpy(b, &v, 8); o.insert(o.end(), b, b + 8); }

    // the runs by (reference, bin), file order inside a bin
    std::vector<size_t> by_bin() const
    {
        std::vector<size_t> order(runs.size());
        for (size_t k = 0; k < order.size(); k++) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            return runs[a].ref != runs[b].ref ? runs[a].ref < runs[b].ref : runs[a].bin < runs[b].bin; });
        return order;
    }

    // the distinct (ref, bin) of the runs, ascending: {ref, bin} pairs back to back - what k_index_loff is launched over
    std::vector<uint32_t> pairs() const
    {
        const std::vector<size_t> order = by_bin();
        std::vector<uint32_t> p;
        for (size_t k = 0; k < order.size(); k++) {
            const IxRun& r = runs[order[k]];
            if (k && runs[order[k - 1]].ref == r.ref && runs[order[k - 1]].bin == r.bin) continue;
            p.push_back((uint32_t)r.ref); p.push_back(r.bin);
        }
        return p;
    }

    // the payload of a .csi file (csi_index.h restates the format): no linear index - a bin carries its loffset, the filled linear
    // entry of its first deepest-level window; the pseudo-bin last per reference; n_no_coor behind the last reference
    std::vector<uint8_t> bytes_csi() const
    {
        std::vector<uint8_t> o;
        o.insert(o.end(), {'C', 'S', 'I', 1});
        put32(o, (uint32_t)fmt.min_shift); put32(o, (uint32_t)fmt.depth); put32(o, 0u);          // l_aux: 0 for BAM
        put32(o, (uint32_t)n_ref);
        const std::vector<size_t> order = by_bin();
        std::vector<ix_i64> first((size_t)n_ref, -1), last((size_t)n_ref, -1);
        for (size_t k = 0; k < runs.size(); k++) { if (first[(size_t)runs[k].ref] < 0) first[(size_t)runs[k].ref] = (ix_i64)k; last[(size_t)runs[k].ref] = (ix_i64)k; }
        std::vector<ix_u64> fill;
        size_t at = 0, pair = 0;
        for (int32_t r = 0; r < n_ref; r++) {
            size_t e = at;
            uint32_t n_bin = 0;
            while (e < order.size() && runs[order[e]].ref == r) { if (e == at || runs[order[e]].bin != runs[order[e - 1]].bin) n_bin++; e++; }
            const bool has = first[(size_t)r] >= 0;
            put32(o, n_bin + (has ? 1u : 0u));
            const ix_i64 n_lin = lin_off[(size_t)r + 1] - lin_off[(size_t)r];
            if (!has_loff && n_bin) {                                // an empty window takes the entry of the next window that has one
                const ix_u64* io = lin.data() + lin_off[(size_t)r];
                fill.assign((size_t)n_lin, 0);
                ix_u64 next = 0;
                for (ix_i64 w = n_lin - 1; w >= 0; w--) { if (io[w] != IX_NONE) next = io[w]; fill[(size_t)w] = next; }
            }
            for (size_t k = at; k < e;) {
                size_t j = k;
                while (j < e && runs[order[j]].bin == runs[order[k]].bin) j++;
                const uint32_t bin = runs[order[k]].bin;
                const ix_i64 bot = ix_bin_bot(bin, fmt);
                ix_u64 lo = 0;
                if (has_loff) lo = pair < loff.size() ? loff[pair] : 0;
                else if (bot >= 0 && bot < n_lin) lo = fill[(size_t)bot];
                pair++;
                put32(o, bin); put64(o, lo); put32(o, (uint32_t)(j - k));
                for (; k < j; k++) { put64(o, runs[order[k]].beg); put64(o, runs[order[k]].end); }
            }
            at = e;
            if (has) {
                put32(o, ix_pseudo_bin(fmt)); put64(o, 0); put32(o, 2u);
                put64(o, runs[(size_t)first[(size_t)r]].beg); put64(o, runs[(size_t)last[(size_t)r]].end);
                put64(o, counts[2 * (size_t)r]); put64(o, counts[2 * (size_t)r + 1]);
            }
        }
        put64(o, counts[2 * (size_t)n_ref]);
        return o;
    }

    std::vector<uint8_t> bytes() const
    {
        std::vector<uint8_t> o;
        o.insert(o.end(), {'B', 'A', 'I', 1});
        put32(o, (uint32_t)n_ref);
        const std::vector<size_t> order = by_bin();
        // the first and the last run of a reference in FILE order: the pseudo-bin's pair
        std::vector<ix_i64> first((size_t)n_ref, -1), last((size_t)n_ref, -1);
        for (size_t k = 0; k < runs.size(); k++) { if (first[(size_t)runs[k].ref] < 0) first[(size_t)runs[k].ref] = (ix_i64)k; last[(size_t)runs[k].ref] = (ix_i64)k; }
        size_t at = 0;
        for (int32_t r = 0; r < n_ref; r++) {
            size_t e = at;
            uint32_t n_bin = 0;
            while (e < order.size() && runs[order[e]].ref == r) { if (e == at || runs[order[e]].bin != runs[order[e - 1]].bin) n_bin++; e++; }
            const bool has = first[(size_t)r] >= 0;
            put32(o, n_bin + (has ? 1u : 0u));
            for (size_t k = at; k < e;) {
                size_t j = k;
                while (j < e && runs[order[j]].bin == runs[order[k]].bin) j++;
                put32(o, runs[order[k]].bin); put32(o, (uint32_t)(j - k));
                for (; k < j; k++) { put64(o, runs[order[k]].beg); put64(o, runs[order[k]].end); }
            }
            at = e;
            if (has) {
                put32(o, IX_PSEUDO_BIN); put32(o, 2u);
                put64(o, runs[(size_t)first[(size_t)r]].beg); put64(o, runs[(size_t)last[(size_t)r]].end);
                put64(o, counts[2 * (size_t)r]); put64(o, counts[2 * (size_t)r + 1]);
            }
            // n_intv: the last touched window + 1; an empty window takes the entry of the next window that has one
            const ix_u64* io = lin.data() + lin_off[(size_t)r];
            ix_i64 n_intv = lin_off[(size_t)r + 1] - lin_off[(size_t)r];
            while (n_intv > 0 && io[n_intv - 1] == IX_NONE) n_intv--;
            put32(o, (uint32_t)n_intv);
            const size_t base = o.size();
            o.resize(base + 8 * (size_t)n_intv);
            ix_u64 next = 0;
            for (ix_i64 w = n_intv - 1; w >= 0; w--) {
                if (io[w] != IX_NONE) next = io[w];
                memcpy(o.data() + base + 8 * (size_t)w, &next, 8);
            }
        }
        put64(o, counts[2 * (size_t)n_ref]);
        return o;
    }
};

}  // namespace ix
}  // namespace csv

// ---- The reader's way to the device (stage_index.hip.h), for bam_host.cpp alone: inside the library, not part of the C ABI.
// csv_index_begin uploads the block table and the reference lengths and clears the linear arrays and the counts, which then live in
// device memory for the whole build; csv_index_window indexes the rows csv_frame_run left on the device (they do not come down) and
// hands down the verdict and the runs; csv_index_end downloads the arrays and the counts, once.
struct csv_ctx;
#define INDEX_LOCAL extern "C" __attribute__((visibility("hidden")))
INDEX_LOCAL int csv_index_begin(csv_ctx* c, int32_t n_ref, const csv::ix_i64* l_ref, int64_t n_blocks, const csv::ix_i64* uoff, const csv::ix_i64* coff, const uint32_t* isize);
INDEX_LOCAL int csv_index_window(csv_ctx* c, int64_t n_records, int64_t win_u0, int64_t ordinal0, const csv::IxCarry* carry, csv::IxVerdict* verdict, const csv::IxRun** runs);
INDEX_LOCAL int csv_index_end(csv_ctx* c, csv::ix_u64* lin, int64_t n_lin, csv::ix_u64* counts, int64_t n_counts);
// a CSI build: csv_index_begin_fmt opens it with the scheme (csv_index_begin is the BAI scheme); csv_index_end_loff closes it without the
// linear arrays coming down - pairs: n_pairs {ref, bin} of bins that hold records, each with bin < ix_n_bins and its first window
// inside the reference's entries (checked); k_index_loff writes loff[k], the first touched entry from that window on, IX_NONE: none.
// Weak: a stand-alone host build of bam_host.cpp (tests/bam_host_main.cpp) links without them and a CSI build on the device is refused
#define INDEX_LOCAL_WEAK extern "C" __attribute__((visibility("hidden"), weak))
INDEX_LOCAL_WEAK int csv_index_begin_fmt(csv_ctx* c, const csv::IxFormat* fmt, int32_t n_ref, const csv::ix_i64* l_ref, int64_t n_blocks, const csv::ix_i64* uoff, const csv::ix_i64* coff, const uint32_t* isize);
INDEX_LOCAL_WEAK int csv_index_end_loff(csv_ctx* c, int64_t n_pairs, const uint32_t* pairs, csv::ix_u64* loff, csv::ix_u64* counts, int64_t n_counts);
INDEX_LOCAL_WEAK double csv_index_loff_ms(csv_ctx* c);            // device time of k_index_loff in the last CSI build
INDEX_LOCAL int csv_index_counters(csv_ctx* c, double* ms_kernels, int64_t* bytes_down, int64_t* bytes_up, int64_t* windows);
