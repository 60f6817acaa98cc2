// ref_core.h — reference bases out of the inflated blocks of a BGZF-compressed FASTA, written once for the host and for the device
// (DESIGN.md section 35), and behind them the event core: the .fai of such a text, window by window, from bytes or from event rows.
// Plain C++: no HIP header, no global state.  Three rules of the gather live here and nowhere else:
//   * the address rule: base i of a contig whose first base sits at uncompressed offset base_off, with lb bases per line of lw
//     bytes, lies at base_off + (i / lb) * lw + i % lb (ref_addr) - the .fai arithmetic;
//   * the tile cut: a range of n bases is REF_TILE-base output tiles, ceil(n / REF_TILE) of them (ref_tiles); tile_first is the
//     running sum over the ranges, and ref_last_le finds a tile's range in it;
//   * the block search: the touched blocks are sorted by uncompressed offset and disjoint, so the block of an address is the last
//     one that starts at or before it (ref_last_le again; an empty block shares its offset with its successor and sorts in front of
//     it), and the blocks of the following addresses are found by walking forward.
// ref_tile copies the bases of one tile with the lanes of a `Lanes` policy: RefOneLane (below) is the host form - the twin of the
// device route, the "host" route of fasta.BgzfReference.gather and what tests/ref_core_main.cpp runs under the sanitizers;
// RefWave (bam.hip.h) is the 64 lanes of a wavefront.
//
// Bounds: ref_tile trusts its tables.  ref_covered is the check that earns that trust, made on the host before anything runs: every
// source byte of a range lies inside one of the blocks.  With it, every read of ref_tile is at data_off[k] + (a - uoff[k]) with
// uoff[k] <= a < uoff[k] + isize[k], inside block k's bytes, and the forward walk ends at or before the last block.  A write goes to
// dst[i - i0] with i0 <= i < i1: the tile's own bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define REF_FN __host__ __device__ inline
#else
#define REF_FN inline
#endif

namespace csv {

typedef long long ref_i64;

constexpr int REF_TILE = 4096;      // bases per output tile: a DEL of 10^6 bases is 245 wavefronts' work, not one's

// the inflated bytes of the touched blocks: block k covers the uncompressed offsets [uoff[k], uoff[k] + isize[k]) and its bytes
// stand at data + data_off[k]
struct RefBlocks {
    int n;
    const ref_i64* uoff; const int* isize; const ref_i64* data_off;
    const uint8_t* data;
};

struct RefOneLane {
    REF_FN int lane() const { return 0; }
    REF_FN int width() const { return 1; }
};

REF_FN ref_i64 ref_addr(ref_i64 base_off, int lb, int lw, ref_i64 i) { return base_off + (i / lb) * lw + i % lb; }

REF_FN ref_i64 ref_tiles(ref_i64 n_bases) { return (n_bases + REF_TILE - 1) / REF_TILE; }

// the last index k of the non-decreasing a[0 .. n) with a[k] <= v; -1 when there is none
REF_FN ref_i64 ref_last_le(const ref_i64* a, ref_i64 n, ref_i64 v)
{
    ref_i64 lo = 0, hi = n;                                       // a[k] <= v below lo, a[k] > v from hi on
    while (lo < hi) {
        const ref_i64 mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// bases [i0, i1) of a contig -> dst[0 .. i1 - i0): the block of the first source byte by search, the later ones by walking
template <class Lanes> REF_FN void ref_tile(const Lanes& L, const RefBlocks& B, ref_i64 base_off, int lb, int lw, ref_i64 i0, ref_i64 i1, uint8_t* dst)
{
    if (i1 <= i0) return;
    ref_i64 k = ref_last_le(B.uoff, B.n, ref_addr(base_off, lb, lw, i0));
    if (k < 0) k = 0;                                             // (never, for a checked range)
    for (ref_i64 i = i0 + L.lane(); i < i1; i += L.width()) {
        const ref_i64 a = ref_addr(base_off, lb, lw, i);
        while (k + 1 < B.n && a >= B.uoff[k] + B.isize[k]) k++;
        dst[i - i0] = B.data[B.data_off[k] + (a - B.uoff[k])];
    }
}

// tile t of the ranges whose tiles tile_first[0 .. n_ranges] counts: its range, then its bases; out_off: where a range's bases start
template <class Lanes> REF_FN void ref_gather_tile(const Lanes& L, const RefBlocks& B, ref_i64 n_ranges, const ref_i64* tile_first, const ref_i64* out_off, const ref_i64* base_off,
                                                   const int* lb, const int* lw, const ref_i64* beg, ref_i64 t, uint8_t* out)
{
    const ref_i64 r = ref_last_le(tile_first, n_ranges, t);
    if (r < 0) return;
    const ref_i64 n = out_off[r + 1] - out_off[r], j0 = (t - tile_first[r]) * REF_TILE, j1 = j0 + REF_TILE < n ? j0 + REF_TILE : n;
    ref_tile(L, B, base_off[r], lb[r], lw[r], beg[r] + j0, beg[r] + j1, out + out_off[r] + j0);
}

// does every source byte of bases [beg, end) lie in a block?  Line run by line run, the blocks walked forward.
inline bool ref_covered(const RefBlocks& B, ref_i64 base_off, int lb, int lw, ref_i64 beg, ref_i64 end)
{
    if (end <= beg) return true;
    ref_i64 k = ref_last_le(B.uoff, B.n, ref_addr(base_off, lb, lw, beg));
    if (k < 0) return false;
    for (ref_i64 i = beg; i < end;) {
        const ref_i64 in_line = i % lb, run = lb - in_line < end - i ? lb - in_line : end - i;
        ref_i64 a = ref_addr(base_off, lb, lw, i);
        const ref_i64 a1 = a + run;
        while (a < a1) {
            while (k + 1 < B.n && a >= B.uoff[k + 1]) k++;
            const ref_i64 be = B.uoff[k] + B.isize[k];
            if (a < B.uoff[k] || a >= be) return false;
            a = be < a1 ? be : a1;
        }
        i += run;
    }
    return true;
}

// ------------------------------------------------------------------------------------ the event core: the .fai of a text seen in windows
// The index rules (csv_fasta_index, vcf_emit.cpp) are rules about whole lines: whether a line is a header, its bytes, its bases (bytes
// less a closing '\r'), whether a line break ends it.  A window of the text is therefore reduced to event rows, one per line that a
// line break inside the window ends AND that matters: the first such line of the window, a header, the line after a header, and any
// line whose (bytes, bases) differ from the line before.  The lines between two rows are copies of the first row's line, so the
// assembler (FaiStream::rows) takes them as a count.  fai_event is the row rule, for a lane of k_fai_events (bam.hip.h) and for
// fai_events_host below, its twin; FaiStream holds the index rules once, fed with bytes (feed) or with rows (rows), in any mix.
// Window-relative positions: a line may begin before the window (a negative start); the carry says what the kernel cannot see.
constexpr ref_i64 FAI_HDR = 1ll << 62;          // in FaiRow::bases: the line is a header
constexpr ref_i64 FAI_NONE = -(1ll << 62);      // no such line break in this window

struct FaiRow { ref_i64 start, bytes, bases; };                   // absolute first byte, bytes without the line break, bases | FAI_HDR
struct FaiCarry { ref_i64 start, first, last; };                  // the line in progress: its absolute first byte, that byte, the last byte seen

// the line [s, e) of the window d that starts at absolute offset base; s < 0: it began in an earlier window
REF_FN FaiRow fai_row(const uint8_t* d, ref_i64 base, const FaiCarry& c, ref_i64 s, ref_i64 e)
{
    const ref_i64 bytes = e - s;
    if (bytes <= 0) return FaiRow{base + s, 0, 0};
    const int first = s >= 0 ? d[s] : (int)c.first, last = e >= 1 ? d[e - 1] : (int)c.last;
    return FaiRow{base + s, bytes, (bytes - (last == '\r' ? 1 : 0)) | (first == '>' ? FAI_HDR : 0)};
}

REF_FN bool fai_matters(const FaiRow& prev, const FaiRow& cur) { return ((prev.bases | cur.bases) & FAI_HDR) != 0 || prev.bytes != cur.bytes || prev.bases != cur.bases; }

// the line that the line break at e ends, and whether it matters; q, q2: the line break before e and the one before that (FAI_NONE:
// not in this window - the line then starts where the carry says)
REF_FN bool fai_event(const uint8_t* d, ref_i64 base, const FaiCarry& c, ref_i64 e, ref_i64 q, ref_i64 q2, FaiRow* row)
{
    const ref_i64 cs = c.start - base;
    *row = fai_row(d, base, c, q == FAI_NONE ? cs : q + 1, e);
    if (q == FAI_NONE) return true;
    return fai_matters(fai_row(d, base, c, q2 == FAI_NONE ? cs : q2 + 1, q), *row);
}

// the line in progress behind the window's last line break `last_nl` (FAI_NONE: the carry's line goes on)
REF_FN FaiCarry fai_tail(const uint8_t* d, ref_i64 n, ref_i64 base, const FaiCarry& c, ref_i64 last_nl)
{
    const ref_i64 ts = last_nl == FAI_NONE ? c.start - base : last_nl + 1;
    return FaiCarry{base + ts, ts < 0 ? c.first : ts < n ? (ref_i64)d[ts] : 0, n > 0 ? (ref_i64)d[n - 1] : c.last};
}

// the host form of k_fai_events: the rows of window d[0 .. n) -> rows[0 .. cap) (the count is returned, whatever cap), the carry behind it
inline ref_i64 fai_events_host(const uint8_t* d, ref_i64 n, ref_i64 base, const FaiCarry& c, FaiRow* rows, ref_i64 cap, FaiCarry* tail)
{
    ref_i64 q = FAI_NONE, q2 = FAI_NONE, k = 0;
    for (ref_i64 p = 0; p < n;) {
        const uint8_t* nl = (const uint8_t*)memchr(d + p, '\n', (size_t)(n - p));
        if (!nl) break;
        const ref_i64 e = nl - d;
        FaiRow r;
        if (fai_event(d, base, c, e, q, q2, &r)) { if (k < cap) rows[k] = r; k++; }
        q2 = q; q = e; p = e + 1;
    }
    *tail = fai_tail(d, n, base, c, q);
    return k;
}

// The index of a text that arrives in windows, as bytes or as event rows.  Entries and verdict are csv_fasta_index's over the whole
// text: a line is judged when its line break arrives, the last one without a line break at finish(); a refusal is kept.
struct FaiStream {
    struct Entry { ref_i64 name_off; int name_len; ref_i64 length, offset; int lb, lw; };
    std::vector<Entry> ent;
    std::string names;
    ref_i64 fed = 0;                       // bytes of the text seen so far
    bool bad = false, in_contig = false, last_short = false;
    // the line in progress
    ref_i64 start = 0, nbytes = 0;
    char first = 0, last = 0;
    bool name_done = false;
    std::string name;

    void add(const char* p, ref_i64 n)     // n > 0 more bytes of the line in progress, none of them a line break
    {
        if (nbytes == 0) { first = p[0]; name.clear(); name_done = false; }
        if (first == '>' && !name_done) {
            ref_i64 k = nbytes == 0 ? 1 : 0;
            const ref_i64 k0 = k;
            while (k < n && p[k] != ' ' && p[k] != '\t' && p[k] != '\r') k++;
            name.append(p + k0, (size_t)(k - k0));
            name_done = k < n;
        }
        last = p[n - 1];
        nbytes += n;
    }
    // a complete line: its first byte at `at`, nb bytes, `bases` of them bases, a header (whose name is `name`) or not
    void line(ref_i64 at, ref_i64 nb, ref_i64 bases, bool hdr, bool has_nl)
    {
        if (hdr) {
            ent.push_back(Entry{(ref_i64)names.size(), (int)name.size(), 0, at + nb + (has_nl ? 1 : 0), 0, 0});
            names += name;
            in_contig = true; last_short = false;
        } else if (!in_contig) {
            if (has_nl && bases != 0) bad = true;                                       // sequence before any header
        } else {
            Entry& e = ent.back();
            const ref_i64 width = nb + (has_nl ? 1 : 0);
            if (bases == 0) last_short = true;                                          // an empty line ends the contig's regular part
            else if (last_short) bad = true;                                            // a longer line after a short one
            else {
                if (e.lb == 0) { if (bases > INT32_MAX || width > INT32_MAX) { bad = true; return; } e.lb = (int)bases; e.lw = (int)width; }
                else if (bases > e.lb) { bad = true; return; }
                if (bases < e.lb || (has_nl && width != e.lw)) last_short = true;
                e.length += bases;
            }
        }
    }
    void line_in_progress(bool has_nl) { line(start, nbytes, nbytes - (nbytes > 0 && last == '\r' ? 1 : 0), nbytes > 0 && first == '>', has_nl); nbytes = 0; }
    // k more lines like row r, each ended by a line break: what k calls of line() would do
    void repeat(const FaiRow& r, ref_i64 k)
    {
        if (k <= 0 || bad) return;
        const ref_i64 bases = r.bases & ~FAI_HDR;
        line(r.start, r.bytes, bases, false, true);                                     // (the first copy: every verdict a copy can bring)
        if (!bad && in_contig && bases != 0 && !last_short) ent.back().length += (k - 1) * bases;
        else if (!bad && in_contig && bases != 0 && k > 1) bad = true;                   // (a second line after a short one)
    }

    bool feed(const char* data, ref_i64 size)
    {
        ref_i64 p = 0;
        while (p < size && !bad) {
            const char* nl = (const char*)memchr(data + p, '\n', (size_t)(size - p));
            const ref_i64 e = nl ? nl - data : size;
            if (nbytes == 0) start = fed + p;
            if (e > p) add(data + p, e - p);
            if (!nl) break;
            line_in_progress(true);
            p = e + 1;
        }
        fed += size;
        return !bad;
    }
    FaiCarry carry() const { return FaiCarry{nbytes > 0 ? start : fed, nbytes > 0 ? (ref_i64)(unsigned char)first : 0, nbytes > 0 ? (ref_i64)(unsigned char)last : 0}; }
    // the next window of n bytes as its event rows, the carry behind it, and the header texts: per header row, then for a header in
    // progress behind the window, the bytes of that line that lie inside the window, back to back.  false: the rows do not describe a
    // window behind this stream's text (nothing is judged from them then), or the text is refused.
    bool rows(const FaiRow* r, ref_i64 n_rows, const char* hdr, ref_i64 hdr_bytes, ref_i64 n, const FaiCarry& tail)
    {
        if (bad) { fed += n; return false; }
        const ref_i64 base = fed, end = fed + n;
        ref_i64 at = carry().start, h = 0;                                              // where the next line starts
        auto header_text = [&](ref_i64 s, ref_i64 e) {                                  // the bytes of the header line [s, e) inside the window
            const ref_i64 s0 = s < base ? base : s, len = e - s0;
            if (len <= 0) return true;
            if (h + len > hdr_bytes) return false;
            if (s0 == s) nbytes = 0;
            start = s;
            add(hdr + h, len);
            h += len;
            return true;
        };
        for (ref_i64 i = 0; i < n_rows && !bad; i++) {
            if (i > 0) {
                const ref_i64 w = r[i - 1].bytes + 1, gap = r[i].start - at;
                if (gap < 0 || gap % w) return false;
                repeat(r[i - 1], gap / w);
                at = r[i].start;
            }
            if (r[i].start != at || r[i].bytes < 0 || r[i].start + r[i].bytes >= end) return false;
            if (r[i].bases & FAI_HDR) {
                if (!header_text(r[i].start, r[i].start + r[i].bytes)) return false;
                line(r[i].start, r[i].bytes, 0, true, true);
            } else line(r[i].start, r[i].bytes, r[i].bases, false, true);
            nbytes = 0;
            at = r[i].start + r[i].bytes + 1;
        }
        if (!bad) {
            if (n_rows > 0) {
                const ref_i64 w = r[n_rows - 1].bytes + 1, gap = tail.start - at;
                if (gap < 0 || gap % w) return false;
                repeat(r[n_rows - 1], gap / w);
            } else if (tail.start != at) return false;
            if (tail.start > end) return false;
            if (tail.start < end) {
                if (tail.first == '>') { if (!header_text(tail.start, end)) return false; }
                else { start = tail.start; nbytes = end - tail.start; first = (char)tail.first; last = (char)tail.last; }
            }
        }
        fed = end;
        return !bad;
    }
    bool finish() { if (!bad && nbytes > 0) line_in_progress(false); return !bad; }
};

}  // namespace csv
