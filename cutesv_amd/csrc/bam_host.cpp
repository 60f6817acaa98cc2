// bam_host.cpp — the host side of the native BAM reader: the BGZF block table, the inflated window, the BAM
// header, the region scan, the two images of a chunk and the index, in that order; the C entry points stand at the end.  The state
// of each concern is one sub-struct of csv_bam, described there.  Three routes share all of it and differ only inside load_window
// and next_host / next_framed: the default - host threads inflate, the host frames; csv_bam_set_inflate - the
// device inflates, the host only the blocks it gave up on; csv_bam_set_frame (section 29) - the window never leaves the device, the
// records are framed there (frame_core.h) and the scan runs over the rows of the record table.  With an index (bai_index.h, section
// 28) a region's scan starts at its linear-index entry; the index moves the starting point and nothing else.  csv_bam_index_build
// (section 30) makes one in a whole-file pass on the reader's routes, through index_core.h.  A .csi (csi_index.h, section 32) is read
// and built as well: index_start / index_stop are the one place that knows which of the two the reader has.  csv_bam_sort (section
// 39) is the other whole-file pass: it assumes nothing about the file's order and writes the records sorted by coordinate, through
// sort_core.h.
//
// Written from the SAM/BAM specification (SAMv1, sections 4.1 "The BGZF compression format" and 4.2 "The BAM format"):
//   BGZF block  = gzip member with one extra subfield 'B','C' (u16 BSIZE = block size - 1), raw deflate payload, CRC32, ISIZE
//   BAM         = "BAM\1", l_text, text, n_ref, {l_name, name, l_ref} * n_ref, then records
//   record      = block_size, then block_size bytes: refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID
//                 next_pos tlen (32 bytes), read_name, cigar (u32 * n_cigar_op), seq ((l_seq + 1) / 2), qual (l_seq), aux
// What goes to the device per record is the slim image {32 fixed bytes, CIGAR words, aux bytes}; the read name and the 4-bit
// sequence stay in the host image; the qualities are dropped.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cutesv_hip.h"
#include "bai_index.h"
#include "csi_index.h"
#include "frame_core.h"
#include "index_core.h"
#include "sort_core.h"

namespace {

typedef int64_t i64;

inline uint32_t rd_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }     // (little-endian hosts only, as the rest of the library)
inline int32_t  rd_i32(const uint8_t* p) { int32_t v; memcpy(&v, p, 4); return v; }
inline uint16_t rd_u16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Block { i64 coff; int32_t csize, hdr; uint32_t isize; i64 uoff; };      // coff: file offset, hdr: bytes before the deflate payload

constexpr int REFILL_BLOCKS = 256;           // BGZF blocks inflated per refill of the window (<= 16 MiB inflated)
constexpr int AHEAD_STEP_BLOCKS = 16;        // ... past the guessed end of an indexed region
constexpr int64_t MAX_LIN_ENTRIES = 1ll << 26; // linear entries of one index build over all references (512 MiB of offsets)
constexpr int MAX_WINDOW_BLOCKS = 16384;     // ... on the device route at most (csv_bam_set_inflate; <= 1 GiB inflated)

}  // namespace

struct csv_bam {
    std::string err;
    struct File {                                // the mapped file and its block table
        int            fd = -1, threads = 1;     // threads: host threads of the inflate
        const uint8_t* map = nullptr;
        i64            size = 0, utotal = 0;     // utotal: bytes of the inflated stream
        std::string    path;
        std::vector<Block> blocks;
    } file;
    struct Header {
        std::string      text, names;            // names: NUL-terminated, back to back
        std::vector<i64> lengths;
        int32_t          n_ref = 0;
        i64              first_rec = 0;          // uncompressed offset of the first record
    } hdr;
    struct Window {                              // the inflated blocks [b0, b1): bytes [u0, u0 + n) of the stream.  n == 0: none
        std::vector<uint8_t> buf;                // (the host route's storage)
        const uint8_t*       p = nullptr;        // the bytes: buf.data(), or the page-locked window; NULL on the framing route
        i64                  n = 0, u0 = 0;
        size_t               b0 = 0, b1 = 0;
    } win;
    // the device inflate route (csv_bam_set_inflate), on which the framing route inflates as well: the context, blocks per window, the
    // page-locked window, the tables of one call, the counters of the last read
    struct DeviceInflate {
        csv_ctx*              ctx = nullptr;
        int                   window_blocks = REFILL_BLOCKS;
        uint8_t*              pin = nullptr;
        i64                   pin_cap = 0;
        std::vector<int64_t>  in_off, out_off;
        std::vector<int32_t>  in_len, out_len;
        std::vector<uint32_t> crc;
        std::vector<uint8_t>  status;            // (in_off .. status: one entry per block of the call, as csv_bgzf_inflate takes them)
        i64                   device_blocks = 0, fallback_blocks = 0;
        double                ms_kernels = 0;
    } dev;
    // the framing route (csv_bam_set_frame): the window lies in the context's device memory and is known here by its rows - the
    // records the chain from `from` met, up to `tail` where it stopped (stream offsets; tail_bs: the block_size there when those 4
    // bytes were inside).  valid: the rows are the window's and lie on the host.  pending: the selected records of the window that
    // are not packed yet; slim_size / host_size: the bytes of the device images with them; chunk: the chunk handed out last is a
    // device chunk, and l_name_v / l_seq_v hold what csv_bam_chunk_lengths says of it
    struct Frame {
        csv_ctx*                 ctx = nullptr;
        uint64_t                 serial = 0;     // the context's window serial when this reader loaded its window
        const csv::FrRow*        rows = nullptr;
        i64                      n = 0, i = 0, from = 0, tail = 0;
        int32_t                  tail_bs = 0;
        bool                     tail_has_bs = false, valid = false, chunk = false;
        std::vector<csv::FrPack> pending;
        std::vector<int32_t>     l_name_v, l_seq_v, t_len;
        std::vector<int64_t>     t_off;          // (t_off / t_len: the block table of one csv_frame_run)
        std::vector<uint8_t>     one_block;      // a block the host inflated, on its way up
        i64                      slim_size = 0, host_size = 0;
    } fr;
    struct Scan {                                // where the scan stands, and what earlier scans found
        i64                  cur = 0;            // uncompressed offset of the next record
        std::map<uint32_t, i64> contig_at;       // (uint32)refID -> offset of its first record, as found (-1 sorts last, as in a sorted file)
        uint32_t             scanned_key = 0;    // every contig with a key <= this one that exists is in contig_at
        bool                 scanned_any = false;
        // the last region scan: its first record.  Records before it end at or before hint_beg, so a later region of the same
        // contig that begins at or after hint_beg starts its scan there
        uint32_t             hint_key = 0;
        i64                  hint_beg = 0, hint_at = -1;
        // seek_key: the contig the running scan was positioned in by the index - the first record it sees of that contig is not
        // the contig's first
        bool                 seeked = false;
        uint32_t             seek_key = 0;
        i64                  ahead_block = -1;   // with an index: the block where the running region is guessed to end (-1: no guess)
        size_t               range_i = 0;        // csv_bam_read_ranges: the range the scan is in
    } scan;
    // the index (csv_bam_index_load / csv_bam_index_build): the scan of a region starts at its linear-index entry (a .bai) or at
    // the loffset of the bin at or in front of it (a .csi); index_start / index_stop ask whichever is there.
    // The counts of the pseudo-bins are kept here for either.  built: it was built here - its bytes, as the index file holds them
    // (payload: a .csi's before the BGZF compression), and the counters of the build
    struct Index {
        bool                 has = false, built = false;
        int                  format = CSV_BAM_INDEX_NONE;
        bai::Index           index;
        csi::Index           csi;
        std::vector<uint64_t> n_mapped, n_unmapped;
        uint64_t             n_no_coor = 0;
        bool                 has_no_coor = false;
        std::vector<uint8_t> bytes, payload;
        i64                  records = 0, runs = 0, frame_runs = 0, windows = 0, up = 0, down = 0, bins = 0;
        double               ms_kernels = 0, ms_loff = 0;
    } ix;
    // the last csv_bam_sort / csv_bam_sort_host: its counters and the block table of the file it wrote, the
    // end-of-file block included
    struct Sorted {
        i64                   records = 0, inversions = 0, inflated = 0, stream = 0, out_bytes = 0, blocks = 0, slices = 0, passes = 0, up = 0, down = 0;
        double                ms[4] = {0, 0, 0, 0};          // device time: keys, sort, gather, deflate
        std::vector<i64>      uoff, coff;
        std::vector<uint32_t> isize;
    } so;
    struct Chunk {                               // the chunk handed out last (the host route's images), and what the read cost
        std::vector<uint8_t>  slim, host;
        std::vector<i64>      rec_off, host_off;
        std::vector<uint32_t> rec_len;
        double                ms_inflate = 0;
        i64                   inflated = 0, compressed = 0;
    } chunk;
};

namespace {

int fail(csv_bam* b, int code, const char* fmt, const char* a = "", long long x = 0)
{
    char buf[512];
    snprintf(buf, sizeof buf, fmt, a, x);
    b->err = buf;
    return code;
}

// what a broken record chain says, on every route
int fail_ends_inside(csv_bam* b, i64 u) { return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)u); }
int fail_small_bs(csv_bam* b, i64 u) { return fail(b, CSV_E_INVALID, "%srecord with block_size < 32 at inflated byte %lld", "", (long long)u); }
int fail_framing(csv_bam* b, int rc) { return fail(b, rc, "the device framing failed: %s", csv_last_error(b->fr.ctx)); }

// ---- the file and its blocks
// the block table: one pass over the block headers of the mapped file
int index_blocks(csv_bam* b)
{
    csv_bam::File& f = b->file;
    i64 o = 0, u = 0;
    while (o < f.size) {
        const uint8_t* p = f.map + o;
        if (o + 18 > f.size) return fail(b, CSV_E_INVALID, "%struncated BGZF block header at byte %lld", "", (long long)o);
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return fail(b, CSV_E_INVALID, "%snot a BGZF block at byte %lld", "", (long long)o);
        const int xlen = rd_u16(p + 10);
        if (o + 12 + xlen > f.size) return fail(b, CSV_E_INVALID, "%struncated BGZF block header at byte %lld", "", (long long)o);
        int bsize = -1;
        for (int x = 0; x + 4 <= xlen;) {                  // extra subfields: SI1 SI2 SLEN data
            const uint8_t* s = p + 12 + x;
            const int slen = rd_u16(s + 2);
            if (s[0] == 'B' && s[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = rd_u16(s + 4);
            x += 4 + slen;
        }
        if (bsize < 0) return fail(b, CSV_E_INVALID, "%sBGZF block without a BC subfield at byte %lld", "", (long long)o);
        const i64 total = (i64)bsize + 1;
        if (total < 12 + xlen + 8) return fail(b, CSV_E_INVALID, "%sBGZF block too short at byte %lld", "", (long long)o);
        if (o + total > f.size) return fail(b, CSV_E_INVALID, "%struncated BGZF block at byte %lld", "", (long long)o);
        Block k;
        k.coff = o; k.csize = (int32_t)total; k.hdr = 12 + xlen; k.isize = rd_u32(p + total - 4); k.uoff = u;
        if (k.isize > 65536) return fail(b, CSV_E_INVALID, "%sBGZF block inflates to more than 64 KiB at byte %lld", "", (long long)o);
        f.blocks.push_back(k);
        u += k.isize; o += total;
    }
    f.utotal = u;
    if (f.blocks.empty() || f.blocks.back().isize != 0 || f.blocks.back().csize != 28)
        return fail(b, CSV_E_INVALID, "%sthe BGZF end-of-file block is missing (truncated file?)", "");
    return CSV_OK;
}

size_t block_of(const csv_bam* b, i64 u)                  // the block that holds uncompressed offset u (u < utotal)
{
    const std::vector<Block>& blocks = b->file.blocks;
    size_t lo = 0, hi = blocks.size();
    while (hi - lo > 1) { const size_t m = (lo + hi) / 2; if (blocks[m].uoff <= u) lo = m; else hi = m; }
    while (lo + 1 < blocks.size() && blocks[lo].isize == 0) lo++;
    return lo;
}

// the block a virtual offset of the (validated) index points into -> the offset in the inflated stream
i64 stream_offset(const csv_bam* b, uint64_t voff, size_t* block)
{
    const std::vector<Block>& blocks = b->file.blocks;
    const i64 coff = (i64)(voff >> 16);
    size_t lo = 0, hi = blocks.size();
    while (hi - lo > 1) { const size_t m = (lo + hi) / 2; if (blocks[m].coff <= coff) lo = m; else hi = m; }
    if (block) *block = lo;
    return blocks[lo].uoff + (i64)(voff & 0xffff);
}

bool inflate_block(const csv_bam* b, const Block& k, uint8_t* dst)
{
    if (k.isize == 0) return true;
    const uint8_t* map = b->file.map;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = const_cast<Bytef*>(map + k.coff + k.hdr);
    z.avail_in = (uInt)(k.csize - k.hdr - 8);
    z.next_out = dst; z.avail_out = k.isize;
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.avail_out == 0;
    inflateEnd(&z);
    if (!ok) return false;
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, k.isize) == rd_u32(map + k.coff + k.csize - 8);
}

// ---- the window
// the host route's inflate: the blocks [b0, b1) into a window that starts at stream offset u0, on the reader's threads
// -> a block inflate_block refuses, or -1
i64 inflate_on_threads(const csv_bam* b, size_t b0, size_t b1, uint8_t* win, i64 u0)
{
    const std::vector<Block>& blocks = b->file.blocks;
    std::atomic<size_t> next(b0);
    std::atomic<i64> bad(-1);
    auto work = [&] {
        for (;;) {
            const size_t k = next.fetch_add(8);            // 8 blocks at a time: neighbours stay on one thread
            if (k >= b1) return;
            for (size_t j = k; j < std::min(k + 8, b1); j++)
                if (!inflate_block(b, blocks[j], win + (blocks[j].uoff - u0))) bad.store((i64)j);
        }
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)b->file.threads, (b1 - b0 + 7) / 8));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return bad.load();
}

// the device route's room: a page-locked window of at least `bytes` bytes with the kept tail at its front
int pin_room(csv_bam* b, i64 bytes, i64 keep, i64 keep_at)
{
    csv_bam::DeviceInflate& d = b->dev;
    if (bytes > d.pin_cap) {
        void* p = nullptr;
        const i64 want = bytes + bytes / 4 + 4096;
        if (csv_host_alloc(want, &p) != CSV_OK) return fail(b, CSV_E_NOMEM, "%scannot page-lock an inflate window of %lld bytes", "", (long long)want);
        if (keep > 0) memcpy(p, d.pin + keep_at, (size_t)keep);
        if (d.pin) csv_host_free(d.pin);
        d.pin = (uint8_t*)p; d.pin_cap = want;
    } else if (keep > 0 && keep_at > 0) memmove(d.pin, d.pin + keep_at, (size_t)keep);
    return CSV_OK;
}

// the selected records of the framing route's window are packed out of it into the device images
int frame_flush(csv_bam* b)
{
    if (b->fr.pending.empty()) return CSV_OK;
    const int rc = csv_frame_pack(b->fr.ctx, (int64_t)b->fr.pending.size(), b->fr.pending.data(), b->fr.slim_size, b->fr.host_size);
    b->fr.pending.clear();
    return rc ? fail_framing(b, rc) : CSV_OK;
}

// The window becomes the inflated blocks [b0, b1).  keep > 0: the window already holds the bytes of the blocks [b0, bn) at its end
// (the scan moved on inside it): they are carried to the front and only [bn, b1) is inflated; else bn == b0.  The routes differ in
// three places.  The room, and how the kept tail gets there: the host vector (in place: no fresh pages per refill), the page-locked
// window, or the context's device window, where csv_frame_window carries the tail itself.  The call that inflates: the host
// threads, or the device with the mapped file from the first block's header to the last block's trailer as its `comp` (nothing is
// gathered).  Where a block the device gave up on goes: inflate_block, whose verdict stands, writes it into the page-locked
// window, or into one_block, which is copied up.
int load_window(csv_bam* b, size_t b0, size_t b1, size_t bn, i64 keep)
{
    enum { HOST, DEVICE, FRAME } const route = b->fr.ctx ? FRAME : b->dev.ctx ? DEVICE : HOST;
    const std::vector<Block>& blocks = b->file.blocks;
    csv_bam::DeviceInflate& d = b->dev;
    int rc;
    if (route == FRAME && (rc = frame_flush(b)) != CSV_OK) return rc;        // (the old window's selected records leave it first)
    const double t0 = now_ms();
    const i64 u0 = blocks[b0].uoff, bytes = (b1 < blocks.size() ? blocks[b1].uoff : b->file.utotal) - u0;
    const i64 keep_at = keep > 0 ? u0 - b->win.u0 : 0;       // where the kept bytes lie in the old window
    b->win.n = 0;
    uint8_t* room = nullptr;
    if (route == HOST) {
        if (keep > 0) memmove(b->win.buf.data(), b->win.buf.data() + keep_at, (size_t)keep);
        b->win.buf.resize((size_t)bytes);
        room = b->win.buf.data();
    } else if (route == DEVICE) {
        if ((rc = pin_room(b, bytes, keep, keep_at)) != CSV_OK) return rc;
        room = d.pin;
    } else b->fr.valid = false;
    b->win.u0 = u0;
    const size_t n = b1 > bn ? b1 - bn : 0;                  // the blocks in front of bn are the kept bytes: inflated already
    i64 bad = -1;
    if (route == HOST) bad = inflate_on_threads(b, bn, b1, room, u0);
    else {
        d.in_off.resize(n); d.in_len.resize(n); d.out_off.resize(n); d.out_len.resize(n); d.crc.resize(n); d.status.resize(n);
        const i64 base = n ? blocks[bn].coff : 0, comp_bytes = n ? blocks[b1 - 1].coff + blocks[b1 - 1].csize - base : 0;
        for (size_t j = 0; j < n; j++) {
            const Block& k = blocks[bn + j];
            d.in_off[j] = k.coff + k.hdr - base; d.in_len[j] = k.csize - k.hdr - 8;
            d.out_off[j] = k.uoff - u0; d.out_len[j] = (int32_t)k.isize;
            d.crc[j] = rd_u32(b->file.map + k.coff + k.csize - 8);
        }
        double ms = 0;
        if (route == FRAME) {
            rc = csv_frame_window(b->fr.ctx, b->file.map + base, comp_bytes, (int32_t)n, d.in_off.data(), d.in_len.data(), d.out_off.data(), d.out_len.data(), d.crc.data(), bytes,
                                  keep, keep_at, d.status.data(), &ms);
            if (!rc) b->fr.serial = csv_frame_window_serial(b->fr.ctx);
        } else
            rc = n == 0 ? CSV_OK : csv_bgzf_inflate(d.ctx, b->file.map + base, comp_bytes, (int32_t)n, d.in_off.data(), d.in_len.data(), d.out_off.data(), d.out_len.data(), d.crc.data(),
                                                    room, bytes, 0, d.status.data(), &ms);
        if (rc) return fail(b, rc, "the device inflate failed: %s", csv_last_error(d.ctx));
        d.ms_kernels += ms;
        if (route == FRAME) b->fr.one_block.resize(65536);
        for (size_t j = 0; j < n; j++) {
            if (!d.status[j]) { d.device_blocks++; continue; }
            d.fallback_blocks++;
            if (!inflate_block(b, blocks[bn + j], route == FRAME ? b->fr.one_block.data() : room + d.out_off[j])) { bad = (i64)(bn + j); continue; }
            if (route != FRAME) continue;
            // (the window is not valid to the reader yet, but it is the context's: the block goes where the device would have put it)
            rc = csv_frame_window_put(b->fr.ctx, d.out_off[j], b->fr.one_block.data(), d.out_len[j]);
            if (rc) return fail(b, rc, "the device inflate failed: %s", csv_last_error(d.ctx));
        }
    }
    for (size_t j = bn; j < b1; j++) b->chunk.compressed += blocks[j].csize;
    b->chunk.inflated += bytes - keep;
    b->chunk.ms_inflate += now_ms() - t0;
    if (bad >= 0) return fail(b, CSV_E_INVALID, "%sBGZF block at byte %lld does not inflate (or fails its CRC)", "", (long long)blocks[(size_t)bad].coff);
    b->win.p = room; b->win.n = bytes; b->win.b0 = b0; b->win.b1 = b1;
    return CSV_OK;
}

// the window holds [u, u + need) of the inflated stream afterwards (refilled when it did not); *have = false: the stream ends
// before u + need
int ensure(csv_bam* b, i64 u, i64 need, bool* have)
{
    const std::vector<Block>& blocks = b->file.blocks;
    const csv_bam::Window& w = b->win;
    *have = false;
    if (u + need > b->file.utotal) return CSV_OK;
    if (u < w.u0 || u + need > w.u0 + w.n) {
        const size_t b0 = block_of(b, u);
        size_t b1 = std::min(blocks.size(), b0 + (size_t)(b->dev.ctx ? b->dev.window_blocks : REFILL_BLOCKS));
        if (b->scan.ahead_block >= 0)                        // an indexed region: up to where it is guessed to end, then in small steps
            b1 = std::min(b1, (i64)b0 <= b->scan.ahead_block ? (size_t)b->scan.ahead_block + 1 : b0 + AHEAD_STEP_BLOCKS);
        while (b1 < blocks.size() && blocks[b1].uoff < u + need) b1++;
        // the scan moved on inside the window: the blocks from b0 to the window's end are there already and are not inflated again
        size_t bn = b0;
        i64 keep = 0;
        if (w.n > 0 && u >= w.u0 && u < w.u0 + w.n && w.b1 > b0) {
            bn = w.b1;
            keep = w.u0 + w.n - blocks[b0].uoff;
            if (b1 < bn) b1 = bn;
        }
        const int rc = load_window(b, b0, b1, bn, keep);
        if (rc) return rc;
    }
    *have = true;
    return CSV_OK;
}

// a pointer to [u, u + need) of the inflated stream, refilling the window when it does not hold the range; nullptr with
// *rc = CSV_OK: the stream ends before u + need
const uint8_t* at(csv_bam* b, i64 u, i64 need, int* rc)
{
    bool have;
    *rc = ensure(b, u, need, &have);
    if (*rc || !have) return nullptr;
    return b->win.p + (u - b->win.u0);
}

// ---- the header
int read_header(csv_bam* b)
{
    csv_bam::Header& h = b->hdr;
    int rc;
    const uint8_t* p = at(b, 0, 12, &rc);
    if (rc) return rc;
    if (!p || memcmp(p, "BAM\1", 4) != 0) return fail(b, CSV_E_INVALID, "%snot a BAM file (no BAM\\1 magic)", "");
    const i64 l_text = rd_i32(p + 4);
    if (l_text < 0) return fail(b, CSV_E_INVALID, "%sbad l_text", "");
    p = at(b, 8, l_text + 4, &rc);
    if (rc) return rc;
    if (!p) return fail(b, CSV_E_INVALID, "%sthe file ends inside the BAM header", "");
    h.text.assign((const char*)p, (size_t)l_text);
    while (!h.text.empty() && h.text.back() == '\0') h.text.pop_back();
    h.n_ref = rd_i32(p + l_text);
    if (h.n_ref < 0) return fail(b, CSV_E_INVALID, "%sbad n_ref", "");
    i64 u = 8 + l_text + 4;
    for (int r = 0; r < h.n_ref; r++) {
        p = at(b, u, 4, &rc);
        if (rc) return rc;
        const i64 l_name = p ? rd_i32(p) : -1;
        if (l_name < 1 || l_name > 1 << 20) return fail(b, CSV_E_INVALID, "%sbad reference name length (reference %lld)", "", r);
        p = at(b, u + 4, l_name + 4, &rc);
        if (rc) return rc;
        if (!p) return fail(b, CSV_E_INVALID, "%sthe file ends inside the BAM header", "");
        h.names.append((const char*)p, strnlen((const char*)p, (size_t)l_name));
        h.names.push_back('\0');
        h.lengths.push_back(rd_u32(p + l_name));
        u += 8 + l_name;
    }
    h.first_rec = b->scan.cur = u;
    return CSV_OK;
}

// ---- the scan and the chunk
// One record of the scan, as the selection loop of read_ranges sees it, from either source: the bytes in the host window (p), or a
// row of the device's record table (p == NULL; span is the row's, src the record's offset in the device window)
struct Rec { i64 bs; uint32_t rkey; i64 pos, l_name, n_cig, l_seq, span, src; const uint8_t* p; };

// The reference span of a record's own CIGAR words (M / D / N / = / X), out of its bytes behind block_size: fr_row's rule on the
// host - the words are read inside the record only, whatever n_cigar says.  Where read_ranges calls it the clamp is a no-op:
// fixed_to_aux <= bs was checked first, so all n_cig words lie inside.
i64 cigar_span(const uint8_t* p, i64 bs, i64 l_name, i64 n_cig)
{
    const i64 cg = 32 + l_name;
    i64 n_in = cg <= bs ? (bs - cg) / 4 : 0, span = 0;
    if (n_in > n_cig) n_in = n_cig;
    for (i64 k = 0; k < n_in; k++) {
        const uint32_t w = rd_u32(p + cg + 4 * k), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += w >> 4;
    }
    return span;
}

// the record at the cursor out of the host window.  *end: the stream ends at the cursor.  The checks and their order are the scan's
// own: the file ends inside the record's block_size, block_size < 32, the file ends inside the record
int next_host(csv_bam* b, Rec* r, bool* end)
{
    const i64 cur = b->scan.cur;
    int rc;
    *end = false;
    const uint8_t* p = at(b, cur, 4, &rc);
    if (rc) return rc;
    if (!p) { *end = cur == b->file.utotal; return *end ? CSV_OK : fail_ends_inside(b, cur); }
    const i64 bs = rd_i32(p);
    if (bs < 32) return fail_small_bs(b, cur);
    p = at(b, cur + 4, bs, &rc);
    if (rc) return rc;
    if (!p) return fail_ends_inside(b, cur);
    r->bs = bs; r->rkey = (uint32_t)rd_i32(p); r->pos = rd_i32(p + 4); r->l_name = p[8]; r->n_cig = rd_u16(p + 12); r->l_seq = rd_u32(p + 16);
    r->span = -1; r->src = 0; r->p = p;
    return CSV_OK;
}

// The framing route's step: the device window is loaded so that it holds the record at the cursor, and framed from there, with
// next_host's checks and texts.  at_tail: the chain framed last stopped at the cursor, at a record it could not step over, and
// fr.tail_bs is its block_size.  *end: the stream ends at the cursor.  Otherwise fr.n / from / tail / tail_bs / tail_has_bs describe
// the new chain; want_rows: its rows come down (fr.rows, fr.valid), else they stay on the device for the index kernels.  A chain
// that makes no progress is the caller's to notice.
int frame_step(csv_bam* b, bool at_tail, bool want_rows, bool* end)
{
    csv_bam::Frame& f = b->fr;
    const i64 cur = b->scan.cur, utotal = b->file.utotal;
    i64 need = 4;
    *end = cur == utotal;
    if (*end) return CSV_OK;
    if (cur + 4 > utotal) return fail_ends_inside(b, cur);
    if (at_tail) {
        const i64 bs = f.tail_bs;
        if (bs < 32) return fail_small_bs(b, cur);
        if (cur + 4 + bs > utotal) return fail_ends_inside(b, cur);
        need = 4 + bs;
    }
    if (csv_frame_window_serial(f.ctx) != f.serial) b->win.n = 0;        // (another reader of the context loaded its window since)
    bool have;
    int rc = ensure(b, cur, need, &have);
    if (rc) return rc;
    f.t_off.clear(); f.t_len.clear();
    for (size_t j = b->win.b0; j < b->win.b1; j++) { f.t_off.push_back(b->file.blocks[j].uoff - b->win.u0); f.t_len.push_back((int32_t)b->file.blocks[j].isize); }
    csv::FrStitch R;
    rc = csv_frame_run(f.ctx, (int32_t)f.t_off.size(), f.t_off.data(), f.t_len.data(), b->hdr.n_ref, cur - b->win.u0, want_rows ? &f.rows : nullptr, &R);
    if (rc) return fail_framing(b, rc);
    f.n = R.n_records; f.i = 0; f.from = cur; f.tail = b->win.u0 + R.tail;
    f.tail_bs = R.tail_bs; f.tail_has_bs = R.tail_has_bs != 0; f.valid = want_rows;
    return CSV_OK;
}

// next_host from the rows of the device window: the window is framed from the cursor when its rows do not hold that offset
int next_framed(csv_bam* b, Rec* r, bool* end)
{
    csv_bam::Frame& f = b->fr;
    for (int round = 0; round < 8; round++) {
        const i64 cur = b->scan.cur;
        if (f.valid && (b->win.n == 0 || cur < f.from || cur > f.tail || csv_frame_window_serial(f.ctx) != f.serial)) f.valid = false;
        if (f.valid && cur < f.tail) {
            const i64 o = cur - b->win.u0;
            i64 k = f.i;
            if (!(k < f.n && f.rows[k].off == o)) {
                const csv::FrRow* e = f.rows + f.n;
                k = std::lower_bound(f.rows, e, o, [](const csv::FrRow& x, i64 v) { return x.off < v; }) - f.rows;
            }
            if (k < f.n && f.rows[k].off == o) {
                const csv::FrRow& w = f.rows[k];
                f.i = k + 1;
                r->bs = w.block_size; r->rkey = (uint32_t)w.refid; r->pos = w.pos; r->l_name = w.l_name; r->n_cig = w.n_cigar; r->l_seq = w.l_seq;
                r->span = w.span; r->src = w.off; r->p = nullptr;
                *end = false;
                return CSV_OK;
            }
            f.valid = false;                                 // (not a start of the chain framed last: framed again from here)
        }
        const int rc = frame_step(b, f.valid && f.tail_has_bs, true, end);       // (valid here: cur == tail, where the chain stopped)
        if (rc || *end) return rc;
    }
    return fail(b, CSV_E_INVALID, "%sthe device framing made no progress at inflated byte %lld", "", (long long)b->scan.cur);
}

// A read starts: the chunk handed out last is dead and the counters start over
void begin_read(csv_bam* b)
{
    csv_bam::Chunk& c = b->chunk;
    c.ms_inflate = 0; c.inflated = c.compressed = 0;
    b->dev.device_blocks = b->dev.fallback_blocks = 0; b->dev.ms_kernels = 0;
    c.slim.clear(); c.host.clear(); c.rec_off.clear(); c.host_off.clear(); c.rec_len.clear();
    csv_bam::Frame& f = b->fr;
    f.pending.clear(); f.l_name_v.clear(); f.l_seq_v.clear(); f.slim_size = f.host_size = 0; f.chunk = false;
    if (f.ctx) { csv_frame_chunk_begin(f.ctx, b); csv_frame_counters(f.ctx, nullptr, nullptr, nullptr, nullptr, nullptr, 1); }
}

// the one place that knows which format the reader's index has
bool index_start(const csv_bam::Index& x, int32_t ref, i64 beg, uint64_t* voff)
{
    return x.format == CSV_BAM_INDEX_CSI ? csi::start_offset(x.csi, ref, beg, voff) : bai::start_offset(x.index, ref, beg, voff);
}
bool index_stop(const csv_bam::Index& x, int32_t ref, i64 end, uint64_t* voff)
{
    return x.format == CSV_BAM_INDEX_CSI ? csi::stop_guess(x.csi, ref, end, voff) : bai::stop_guess(x.index, ref, end, voff);
}

// the index positions the scan for range [beg, end) of contig `key`: the cursor moves forward only (never behind `floor`);
// -> false: the index says that no record overlaps any window from beg's on
bool index_seek(csv_bam* b, uint32_t key, i64 beg, i64 end, i64 floor)
{
    csv_bam::Scan& s = b->scan;
    uint64_t v;
    if (!index_start(b->ix, (int32_t)key, beg, &v)) return false;
    const i64 u = (v >> 16) == (uint64_t)b->file.size ? b->file.utotal : stream_offset(b, v, nullptr);
    if (floor < b->hdr.first_rec) floor = b->hdr.first_rec;  // (no offset of an index leads into the header)
    s.cur = u > floor ? u : floor;
    s.seeked = true; s.seek_key = key;                       // (also from `floor`, a hint: the scan that set it was positioned by the index too)
    size_t k = b->file.blocks.size() - 1;
    if (index_stop(b->ix, (int32_t)key, end, &v) && (v >> 16) != (uint64_t)b->file.size) stream_offset(b, v, &k);
    s.ahead_block = (i64)k;
    return true;
}

// csv_bam_read / csv_bam_read_ranges: the records of contig `refid` that overlap one of the sorted, disjoint ranges, in file order
int read_ranges(csv_bam* b, int32_t refid, size_t nr, const int64_t* rbeg, const int64_t* rend, int64_t max_records, int32_t flags, csv_bam_chunk* out)
{
    const double t0 = now_ms();
    memset(out, 0, sizeof *out);
    begin_read(b);
    csv_bam::Scan& s = b->scan;
    csv_bam::Chunk& c = b->chunk;
    csv_bam::Frame& f = b->fr;
    const bool framed = f.ctx != nullptr;
    const bool count_only = (flags & CSV_BAM_COUNT_ONLY) != 0, restart = (flags & CSV_BAM_RESTART) != 0;
    const uint32_t key = (uint32_t)refid;
    const bool indexed = b->ix.has && refid >= 0 && refid < b->hdr.n_ref;
    size_t ri = s.range_i < nr ? s.range_i : nr - 1;
    bool done = false;                                       // the index says that nothing is left to read
    if (restart) {                                           // start of the contig if it was seen, else the last contig start before it
        ri = 0; s.seeked = false; s.ahead_block = -1;
        const i64 hint = s.hint_at >= 0 && s.hint_key == key && rbeg[0] >= s.hint_beg ? s.hint_at : -1;
        if (indexed) {                                       // the linear-index entry of the first window, or the hint when that lies further on
            if (!index_seek(b, key, rbeg[0], rend[0], hint >= 0 ? hint : 0)) done = true;
        } else {
            s.cur = b->hdr.first_rec;
            auto it = s.contig_at.upper_bound(key);
            if (it != s.contig_at.begin()) { --it; s.cur = it->second; }
            if (hint >= 0) s.cur = hint;
        }
        s.hint_at = -1;
    }
    i64 n = 0;
    bool more = false;
    int rc = CSV_OK;
    while (!done) {
        Rec r;
        bool at_end;
        rc = framed ? next_framed(b, &r, &at_end) : next_host(b, &r, &at_end);
        if (rc) return rc;
        if (at_end) { s.scanned_key = 0xffffffffu; s.scanned_any = true; break; }
        const uint8_t* p = r.p;
        const uint32_t rkey = r.rkey;
        const i64 bs = r.bs, pos = r.pos, l_name = r.l_name, n_cig = r.n_cig;
        if (!(s.seeked && rkey == s.seek_key)) {             // (a scan the index positioned does not see the first record of its contig)
            if (!s.contig_at.count(rkey)) s.contig_at[rkey] = s.cur;
            if (!s.scanned_any || rkey > s.scanned_key) { s.scanned_key = rkey; s.scanned_any = true; }
        }
        if (rkey > key) break;                               // the next contig (the unmapped tail sorts last): not consumed
        if (rkey < key) { s.cur += 4 + bs; continue; }
        const csv::FrLayout lay = csv::fr_layout(bs, l_name, n_cig, r.l_seq);
        if (lay.fixed_to_aux > bs) return fail(b, CSV_E_INVALID, "%srecord fields exceed its block_size at inflated byte %lld", "", (long long)s.cur);
        if (pos >= rend[ri]) {                               // sorted: nothing later can start before this range's end - on to the next range
            while (ri < nr && pos >= rend[ri]) ri++;
            if (ri == nr) { ri = nr - 1; break; }
            if (indexed) {
                if (!index_seek(b, key, rbeg[ri], rend[ri], s.cur)) break;
                continue;                                    // (the cursor may have moved: the record is read again)
            }
        }
        if (pos < rbeg[ri]) {                                // overlaps the range only if it reaches past its begin (and then no later one: they are disjoint)
            const i64 span = p ? cigar_span(p, bs, l_name, n_cig) : r.span;      // (the row's on the framing route)
            if (pos + (span ? span : 1) <= rbeg[ri]) { s.cur += 4 + bs; continue; }
        }
        if (n == max_records) { more = true; break; }
        // (every record in front of this one ends at or before the begin of the range it is emitted for: those tested against an
        // earlier range end before that range's begin, those the index jumped over overlap no window from this range's on)
        if (n == 0 && restart) { s.hint_key = key; s.hint_beg = rbeg[ri]; s.hint_at = s.cur; }
        if (!count_only && framed) {                         // the same layout, in the device images: packed when the window is left
            csv::FrPack q{};
            q.src = r.src; q.rec_off = f.slim_size; q.host_off = f.host_size; q.bs = (int32_t)bs; q.l_seq = (uint32_t)r.l_seq; q.n_cig = (uint16_t)n_cig; q.l_name = (uint8_t)l_name;
            f.pending.push_back(q);
            c.rec_off.push_back(f.slim_size); c.rec_len.push_back((uint32_t)lay.slim_len); c.host_off.push_back(f.host_size);
            f.l_name_v.push_back((int32_t)l_name); f.l_seq_v.push_back((int32_t)(uint32_t)r.l_seq);
            f.slim_size += lay.slim_padded;
            f.host_size += lay.host_len;
        } else if (!count_only) {
            const size_t s0 = c.slim.size();
            c.rec_off.push_back((i64)s0); c.rec_len.push_back((uint32_t)lay.slim_len);
            c.slim.resize(s0 + (size_t)lay.slim_padded);
            uint8_t* d = c.slim.data() + s0;
            memcpy(d, p, 32);
            memcpy(d + 32, p + 32 + l_name, (size_t)(4 * n_cig));
            memcpy(d + 32 + 4 * n_cig, p + lay.fixed_to_aux, (size_t)(bs - lay.fixed_to_aux));
            memset(d + lay.slim_len, 0, (size_t)(lay.slim_padded - lay.slim_len));
            const size_t h0 = c.host.size();
            c.host_off.push_back((i64)h0);
            c.host.resize(h0 + (size_t)lay.host_len);
            memcpy(c.host.data() + h0, p + 32, (size_t)l_name);
            memcpy(c.host.data() + h0 + l_name, p + 32 + l_name + 4 * n_cig, (size_t)lay.seq_bytes);
        }
        n++;
        out->record_bytes += 4 + bs;
        s.cur += 4 + bs;
    }
    s.range_i = ri;
    if (framed) {
        rc = frame_flush(b);
        if (rc) return rc;
        if (!count_only) {
            rc = csv_frame_chunk_end(f.ctx, n, c.rec_off.data(), c.rec_len.data(), c.host_off.data(), f.l_name_v.data(), f.l_seq_v.data());
            if (rc) return fail_framing(b, rc);
            f.chunk = true;
        }
    }
    c.host_off.push_back(framed ? f.host_size : (i64)c.host.size());
    out->n_records = n; out->more = more ? 1 : 0;
    out->slim = framed ? nullptr : c.slim.data(); out->slim_bytes = framed ? f.slim_size : (int64_t)c.slim.size();
    out->rec_off = c.rec_off.data(); out->rec_len = c.rec_len.data();
    out->host = framed ? nullptr : c.host.data(); out->host_bytes = framed ? f.host_size : (int64_t)c.host.size(); out->host_off = c.host_off.data();
    out->inflated_bytes = c.inflated; out->compressed_bytes = c.compressed;
    out->ms_inflate = c.ms_inflate; out->ms_frame = now_ms() - t0 - c.ms_inflate;
    return CSV_OK;
}

// ---- the index: loading, and the build (index_core.h)
bool read_file(const std::string& path, std::vector<uint8_t>* data)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) data->insert(data->end(), buf, buf + k);
    const bool ok = !ferror(f);
    fclose(f);
    return ok;
}

int voff_check(void* user, uint64_t voff)
{
    const csv_bam* b = (const csv_bam*)user;
    const i64 coff = (i64)(voff >> 16);
    if (coff == b->file.size) return (voff & 0xffff) ? 2 : 0;     // "behind the last block": where a writer stands after its end-of-file block
    size_t k;
    stream_offset(b, voff, &k);
    if (b->file.blocks[k].coff != coff) return 1;
    return (voff & 0xffff) > b->file.blocks[k].isize ? 2 : 0;
}

// a parsed and validated index becomes the reader's (csv_bam_index_drop is the counterpart).  built: the bytes it was parsed from,
// kept for csv_bam_index_bytes; NULL: it came from a file.  What earlier scans guessed with another index, or none, is forgotten
void install_common(csv_bam* b, int format, std::vector<uint8_t>* built)
{
    b->ix.format = format;
    b->ix.has = true; b->ix.built = built != nullptr;
    if (built) b->ix.bytes = std::move(*built); else b->ix.bytes.clear();
    b->ix.payload.clear();
    b->scan.hint_at = -1; b->scan.ahead_block = -1;
}

template <class Refs> void keep_counts(csv_bam::Index& x, const Refs& refs, uint64_t n_no_coor, bool has_no_coor)
{
    x.n_mapped.clear(); x.n_unmapped.clear();
    for (const auto& R : refs) { x.n_mapped.push_back(R.n_mapped); x.n_unmapped.push_back(R.n_unmapped); }
    x.n_no_coor = n_no_coor; x.has_no_coor = has_no_coor;
}

void install_index(csv_bam* b, bai::Index&& ix, std::vector<uint8_t>* built)
{
    keep_counts(b->ix, ix.refs, ix.n_no_coor, ix.has_no_coor);
    b->ix.index = std::move(ix);
    b->ix.csi = csi::Index();
    install_common(b, CSV_BAM_INDEX_BAI, built);
}

// ... a .csi's: built: the file's bytes, with the payload they inflate to
void install_index(csv_bam* b, csi::Index&& ix, std::vector<uint8_t>* built, std::vector<uint8_t>* payload)
{
    keep_counts(b->ix, ix.refs, ix.n_no_coor, ix.has_no_coor);
    b->ix.csi = std::move(ix);
    b->ix.index = bai::Index();
    install_common(b, CSV_BAM_INDEX_CSI, built);
    if (payload) b->ix.payload = std::move(*payload);
}

// an index file that is BGZF-compressed as a whole -> its payload, with the reader's own block walk and inflate
bool inflate_index_file(const std::vector<uint8_t>& data, const std::string& name, std::vector<uint8_t>* payload, std::string* err)
{
    csv_bam f;
    f.file.map = data.data(); f.file.size = (i64)data.size();
    if (index_blocks(&f) != CSV_OK) { *err = name + ": " + f.err; return false; }
    payload->resize((size_t)f.file.utotal);
    for (const Block& k : f.file.blocks)
        if (!inflate_block(&f, k, payload->data() + k.uoff)) {
            *err = name + ": the BGZF block at byte " + std::to_string((long long)k.coff) + " does not inflate";
            return false;
        }
    return true;
}

// does the file begin like a BGZF block?  A .bai begins "BAI\1"; what is BGZF-compressed as a whole is taken for a .csi, whose parser
// then asks for the CSI magic in the payload
bool looks_like_bgzf(const std::vector<uint8_t>& data)
{
    return data.size() >= 18 && data[0] == 0x1f && data[1] == 0x8b && data[2] == 8 && (data[3] & 4) && data[12] == 'B' && data[13] == 'C';
}

// payload -> the bytes of the .csi file: BGZF blocks of at most 0xff00 bytes each, and the end-of-file block
bool bgzf_compress(const std::vector<uint8_t>& payload, std::vector<uint8_t>* out)
{
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    out->clear();
    std::vector<uint8_t> z_out(0x10000 + 1024);
    for (size_t at = 0; at <= payload.size();) {
        const size_t len = at < payload.size() ? std::min<size_t>(payload.size() - at, 0xff00) : 0;      // (len 0: the end-of-file block)
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        z.next_in = const_cast<Bytef*>(payload.data() + (len ? at : 0)); z.avail_in = (uInt)len;
        z.next_out = z_out.data(); z.avail_out = (uInt)z_out.size();
        const int rc = deflate(&z, Z_FINISH);
        const size_t clen = z_out.size() - z.avail_out;
        deflateEnd(&z);
        if (rc != Z_STREAM_END || clen + 26 > 0x10000) return false;         // (0xff00 bytes never deflate to more than 64 KiB - 26)
        const uint16_t bsize = (uint16_t)(clen + 25);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), payload.data() + (len ? at : 0), (uInt)len), isize = (uint32_t)len;
        out->insert(out->end(), head, head + 16);
        out->push_back((uint8_t)(bsize & 0xff)); out->push_back((uint8_t)(bsize >> 8));
        out->insert(out->end(), z_out.data(), z_out.data() + clen);
        uint8_t tail[8];
        memcpy(tail, &crc, 4); memcpy(tail + 4, &isize, 4);
        out->insert(out->end(), tail, tail + 8);
        if (len == 0) break;
        at += len;
    }
    return true;
}

struct IxTables { std::vector<csv::ix_i64> uoff, coff, l_ref; std::vector<uint32_t> isize; };

int index_refuse(csv_bam* b, long long ordinal, int why, const csv::ix::Builder& B)
{
    char buf[384];
    snprintf(buf, sizeof buf, "cannot build the index: record %lld %s", ordinal, csv::ix::refusal_text(why, B.fmt, B.csi).c_str());
    b->err = buf;
    return CSV_E_INVALID;
}

// the host routes: every record through the core, one by one
int index_build_host(csv_bam* b, const IxTables& T, csv::ix::Builder* B)
{
    const csv::IxBlocks blocks{T.uoff.data(), T.coff.data(), T.isize.data(), (csv::ix_i64)T.uoff.size()};
    for (;;) {
        Rec r;
        bool at_end;
        const int rc = next_host(b, &r, &at_end);
        if (rc) return rc;
        if (at_end) return CSV_OK;
        const csv::IxRec x = csv::ix_record(r.pos, cigar_span(r.p, r.bs, r.l_name, r.n_cig), B->fmt);
        const int why = csv::ix_refuse((int32_t)r.rkey, r.pos, x, b->hdr.n_ref, T.l_ref.data(), B->prev, B->fmt);
        if (why) return index_refuse(b, B->records, why, *B);
        B->add_record((int32_t)r.rkey, r.pos, x, (rd_u16(r.p + 14) & 4) != 0, csv::ix_voff(blocks, b->scan.cur), csv::ix_voff(blocks, b->scan.cur + 4 + r.bs));
        b->scan.cur += 4 + r.bs;
    }
}

// the framing route: window by window, the rows stay on the device (frame_step without rows) and the index kernels read them
// there; the verdict and the runs come down.  csi: at the end k_index_loff gathers one loffset per bin from the linear arrays, which
// then stay on the device
int index_build_device(csv_bam* b, const IxTables& T, csv::ix::Builder* B)
{
    const bool csi = B->csi;
    csv_ctx* ctx = b->fr.ctx;
    if (csi && (!csv_index_begin_fmt || !csv_index_end_loff)) return fail(b, CSV_E_STATE, "%sthis build of the reader has no device route for a CSI index", "");
    int rc = csi ? csv_index_begin_fmt(ctx, &B->fmt, b->hdr.n_ref, T.l_ref.data(), (int64_t)T.uoff.size(), T.uoff.data(), T.coff.data(), T.isize.data())
                 : csv_index_begin(ctx, b->hdr.n_ref, T.l_ref.data(), (int64_t)T.uoff.size(), T.uoff.data(), T.coff.data(), T.isize.data());
    if (rc) return fail(b, rc, "the device index build failed: %s", csv_last_error(ctx));
    csv::IxCarry carry{0, 0, 0, 0};
    bool at_tail = false;
    int idle = 0;
    b->fr.valid = false;
    for (;;) {
        const i64 cur = b->scan.cur;
        bool at_end;
        rc = frame_step(b, at_tail, false, &at_end);
        if (rc) return rc;
        if (at_end) break;
        b->ix.frame_runs++;
        if (b->fr.n > 0) {
            csv::IxVerdict V;
            const csv::IxRun* runs = nullptr;
            rc = csv_index_window(ctx, b->fr.n, b->win.u0, B->records, &carry, &V, &runs);
            if (rc) return fail(b, rc, "the device index build failed: %s", csv_last_error(ctx));
            if (V.bad != csv::IX_NONE) return index_refuse(b, (long long)(V.bad >> 3), (int)(V.bad & 7), *B);
            for (i64 k = 0; k < V.n_runs; k++) B->add_run(runs[k]);
            b->ix.runs += V.n_runs;
            B->records += b->fr.n;
            carry = V.last;
        }
        if (b->fr.tail > cur) idle = 0;
        else if (++idle > 4) return fail(b, CSV_E_INVALID, "%sthe device framing made no progress at inflated byte %lld", "", (long long)cur);
        at_tail = b->fr.tail_has_bs;
        b->scan.cur = b->fr.tail;
    }
    if (csi) {
        const std::vector<uint32_t> pairs = B->pairs();
        B->loff.assign(pairs.size() / 2, csv::IX_NONE);
        B->has_loff = true;
        rc = csv_index_end_loff(ctx, (int64_t)B->loff.size(), pairs.data(), B->loff.data(), B->counts.data(), (int64_t)B->counts.size());
        if (!rc)
            for (size_t k = 0; k < B->loff.size(); k++)          // (a bin that holds records has a touched window inside its span)
                if (B->loff[k] == csv::IX_NONE) return fail(b, CSV_E_INVALID, "%sthe device index build found no linear entry for bin %lld", "", (long long)pairs[2 * k + 1]);
    } else rc = csv_index_end(ctx, B->lin.data(), (int64_t)B->lin.size(), B->counts.data(), (int64_t)B->counts.size());
    if (rc) return fail(b, rc, "the device index build failed: %s", csv_last_error(ctx));
    return CSV_OK;
}

// ---- the coordinate sort (sort_core.h)
}  // namespace
// (weak, as sort_core.h's device entries are: the host form's compressor lives in bgzf_host.cpp, which a stand-alone build of this file leaves out)
extern "C" __attribute__((weak)) int csv_bgzf_deflate_host(const uint8_t* in, int64_t in_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, uint8_t* out,
                                                          int64_t out_cap, int32_t* block_bytes, int64_t* out_bytes, int32_t* coding_bytes);
namespace {
// Where the inflated stream goes while the pass walks the file: the device arena of `ctx`, or - the host form - a host vector.  Both
// hold the stream at its own offsets, so a record's start in the stream is its start there.  hi: everything below it has arrived
struct SortSink { csv_ctx* ctx; std::vector<uint8_t>* host; i64 hi; };

int fail_sort_device(csv_bam* b, csv_ctx* ctx, int rc) { return fail(b, rc, "the device sort failed: %s", csv_last_error(ctx)); }

// the bytes of the reader's window that the sink does not have yet.  Windows only move forward and begin at the block of the cursor,
// which lies at or below hi: what a window skips at its front is header bytes in front of the first record
int sort_take(csv_bam* b, SortSink* S)
{
    const i64 w_end = b->win.u0 + b->win.n;
    if (b->win.n <= 0 || w_end <= S->hi) return CSV_OK;
    if (b->win.u0 > S->hi && S->hi > b->hdr.first_rec) return fail(b, CSV_E_INVALID, "%sthe sort lost the bytes in front of inflated byte %lld", "", (long long)b->win.u0);
    const i64 from = std::max(S->hi, b->win.u0), len = w_end - from;
    if (S->ctx) {
        const int rc = csv_sort_append(S->ctx, from, b->fr.ctx ? nullptr : b->win.p + (from - b->win.u0), from - b->win.u0, len);
        if (rc) return fail_sort_device(b, S->ctx, rc);
    } else memcpy(S->host->data() + from, b->win.p + (from - b->win.u0), (size_t)len);
    S->hi = w_end;
    return CSV_OK;
}

// Every record start of the file, window by window on the reader's routes, while the windows' bytes go to the sink.  The pass assumes
// nothing about the file's order: it never stops at a record, only at the stream's end.  The framing route takes the starts from
// frame_step's rows; the others step from block_size to block_size with next_host's checks and texts - but ask for the record from
// its first byte on, so that a refill never drops the block in which the record began before the sink has it.
int sort_collect(csv_bam* b, SortSink* S, std::vector<csv::so_i64>* starts)
{
    int rc;
    if (b->fr.ctx) {
        bool at_tail = false;
        int idle = 0;
        b->fr.valid = false;
        for (;;) {
            const i64 cur = b->scan.cur;
            bool at_end;
            if ((rc = frame_step(b, at_tail, true, &at_end)) != CSV_OK) return rc;
            if (at_end) return CSV_OK;
            if ((rc = sort_take(b, S)) != CSV_OK) return rc;
            for (i64 k = 0; k < b->fr.n; k++) starts->push_back(b->win.u0 + b->fr.rows[k].off);
            if (b->fr.tail > cur) idle = 0;
            else if (++idle > 4) return fail(b, CSV_E_INVALID, "%sthe device framing made no progress at inflated byte %lld", "", (long long)cur);
            at_tail = b->fr.tail_has_bs;
            b->scan.cur = b->fr.tail;
        }
    }
    for (;;) {
        const i64 cur = b->scan.cur;
        const uint8_t* p = at(b, cur, 4, &rc);
        if (rc) return rc;
        if (!p) return cur == b->file.utotal ? CSV_OK : fail_ends_inside(b, cur);
        if ((rc = sort_take(b, S)) != CSV_OK) return rc;
        const i64 bs = rd_i32(p);
        if (bs < 32) return fail_small_bs(b, cur);
        p = at(b, cur, 4 + bs, &rc);
        if (rc) return rc;
        if (!p) return fail_ends_inside(b, cur);
        if ((rc = sort_take(b, S)) != CSV_OK) return rc;
        starts->push_back(cur);
        b->scan.cur = cur + 4 + bs;
    }
}

// the BAM header as the file holds it: the blocks in front of the first record, inflated on the host whatever the routes are
int sort_raw_header(csv_bam* b, std::vector<uint8_t>* head)
{
    std::vector<uint8_t> buf;
    for (const Block& k : b->file.blocks) {
        if (k.uoff >= b->hdr.first_rec) break;
        buf.resize((size_t)(k.uoff + k.isize));
        if (!inflate_block(b, k, buf.data() + k.uoff)) return fail(b, CSV_E_INVALID, "%sBGZF block at byte %lld does not inflate (or fails its CRC)", "", (long long)k.coff);
    }
    if ((i64)buf.size() < b->hdr.first_rec) return fail(b, CSV_E_INVALID, "%sthe file ends inside the BAM header", "");
    head->assign(buf.begin(), buf.begin() + b->hdr.first_rec);
    return CSV_OK;
}

// csv_bam_sort (ctx) and csv_bam_sort_host (ctx NULL): one body.  The routes differ in where the stream is collected, in who computes
// keys, order and dst, and in who fills and compresses a slice; the rules are sort_core.h's on both, and csv_bgzf_deflate_host gives
// the device compressor's bytes: the files are equal byte for byte.
int sort_run(csv_bam* b, csv_ctx* ctx, const char* out_path, int64_t max_bytes, int32_t slice_blocks)
{
    if (ctx ? !csv_sort_begin : !csv_bgzf_deflate_host) return fail(b, CSV_E_STATE, "this build of the reader has no %s route for the sort", ctx ? "device" : "host");
    csv_bam::Sorted& so = b->so;
    so = csv_bam::Sorted();
    csv_bam::Scan& s = b->scan;
    begin_read(b);                                           // the sort is a read; the scan state of a region is forgotten as well
    s.seeked = false; s.ahead_block = -1; s.hint_at = -1; s.range_i = 0;
    const i64 slice_bytes = (i64)(slice_blocks > 0 ? slice_blocks : csv::SORT_SLICE_BLOCKS) * csv::SORT_BLOCK;
    const i64 inflated = b->file.utotal, need = inflated + slice_bytes;
    so.inflated = inflated;
    int rc;
    // the budget, before the first window is read
    i64 budget = max_bytes;
    if (ctx && budget <= 0) {
        int64_t free_bytes = 0;
        if ((rc = csv_sort_free_bytes(ctx, &free_bytes)) != CSV_OK) return fail_sort_device(b, ctx, rc);
        budget = free_bytes / 2;
    }
    if (budget > 0 && need > budget) {
        char buf[384];
        snprintf(buf, sizeof buf, "cannot sort: the inflated stream (%lld bytes) and one slice (%lld bytes) take %lld bytes, the budget is %lld bytes; files beyond it are not sorted here (samtools sort)",
                 (long long)inflated, (long long)slice_bytes, (long long)need, (long long)budget);
        b->err = buf;
        return CSV_E_CAPACITY;
    }
    std::vector<uint8_t> head, hdr, arena_h, slice_h, image;
    std::vector<csv::so_i64> starts, dst;                    // (so_i64: the core's 64-bit integer, int64_t's size)
    static_assert(sizeof(csv::so_i64) == sizeof(int64_t), "the starts table is handed on as it is");
    std::vector<int32_t> perm, sizes;
    std::vector<uint64_t> keys;
    if ((rc = sort_raw_header(b, &head)) != CSV_OK) return rc;
    if (!csv::sort_header(head.data(), (i64)head.size(), &hdr)) return fail(b, CSV_E_INVALID, "%scannot sort: the BAM header cannot be rewritten", "");
    const i64 H = (i64)hdr.size();
    FILE* f = nullptr;
    bool opened = false;                                     // a sort is open on the context
    auto finish = [&](int code) {                            // every way out: the context's arena goes back, a failed sort leaves no file
        if (opened) csv_sort_end(ctx);
        if (f) { if (fclose(f) != 0 && !code) code = fail(b, CSV_E_INVALID, "cannot write %s", out_path); if (code) remove(out_path); }
        s.cur = b->hdr.first_rec;
        b->win.n = 0; b->fr.valid = false;                   // (what a later read costs does not depend on what the sort left in the window)
        return code;
    };
    try {
        if (!ctx) arena_h.resize((size_t)inflated + 8);
        slice_h.resize(ctx ? 0 : (size_t)slice_bytes);
        image.resize((size_t)(slice_bytes + 31 * (slice_bytes / csv::SORT_BLOCK)));
        sizes.resize((size_t)(slice_bytes / csv::SORT_BLOCK));
    } catch (const std::bad_alloc&) { return fail(b, CSV_E_NOMEM, "%scannot sort: no memory for the inflated stream (%lld bytes)", "", (long long)inflated); }
    if (ctx) {
        if ((rc = csv_sort_begin(ctx, inflated, hdr.data(), H, slice_bytes)) != CSV_OK) return finish(fail_sort_device(b, ctx, rc));
        opened = true;
    }
    // the windows and the record starts
    SortSink S{ctx, &arena_h, 0};
    s.cur = b->hdr.first_rec;
    b->win.n = 0; b->fr.valid = false;
    try {
        rc = sort_collect(b, &S, &starts);
    } catch (const std::bad_alloc&) { rc = fail(b, CSV_E_NOMEM, "%scannot sort: no memory for the table of record starts (%lld records so far)", "", (long long)starts.size()); }
    if (rc) return finish(rc);
    const i64 n = (i64)starts.size();
    for (i64 i = 0; i < n; i++)                              // (the chain: what every later step relies on)
        if (starts[(size_t)i] < b->hdr.first_rec || starts[(size_t)i] > inflated - 36 || (i && starts[(size_t)i] < starts[(size_t)i - 1] + 36))
            return finish(fail(b, CSV_E_INVALID, "%scannot sort: the chain of records breaks at record %lld", "", (long long)i));
    // keys, verdict, order, dst
    uint64_t bad = csv::SORT_NONE;
    i64 record_bytes = 0;
    if (ctx) {
        csv_sort_verdict V;
        if ((rc = csv_sort_order(ctx, n, (const int64_t*)starts.data(), b->hdr.n_ref, &V)) != CSV_OK) return finish(fail_sort_device(b, ctx, rc));
        bad = V.bad; so.inversions = V.inversions; so.passes = V.passes; record_bytes = V.record_bytes;
    } else {
        try { keys.resize((size_t)n); perm.resize((size_t)n); dst.resize((size_t)n + 1); }
        catch (const std::bad_alloc&) { return finish(fail(b, CSV_E_NOMEM, "%scannot sort: no memory for the tables of %lld records", "", (long long)n)); }
        for (i64 i = 0; i < n; i++) {
            const csv::SortFields fl = csv::sort_fields(arena_h.data() + starts[(size_t)i]);
            const int why = csv::sort_refuse(fl, b->hdr.n_ref);
            if (why) { bad = (uint64_t)i << 3 | (uint64_t)why; break; }
            keys[(size_t)i] = csv::sort_key(fl, b->hdr.n_ref);
            if (i && keys[(size_t)i] < keys[(size_t)i - 1]) so.inversions++;
            perm[(size_t)i] = (int32_t)i;
        }
        if (bad == csv::SORT_NONE) {
            std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return keys[(size_t)x] < keys[(size_t)y]; });
            for (i64 r = 0; r < n; r++) { dst[(size_t)r] = record_bytes; record_bytes += csv::sort_fields(arena_h.data() + starts[(size_t)perm[(size_t)r]]).len; }
            dst[(size_t)n] = record_bytes;
        }
    }
    if (bad != csv::SORT_NONE) {
        const int why = (int)(bad & 7);
        if (why == csv::SORT_WHY_CHAIN) return finish(fail(b, CSV_E_INVALID, "%scannot sort: record %lld is not the record the reader stepped over", "", (long long)(bad >> 3)));
        char buf[384];
        snprintf(buf, sizeof buf, "cannot sort: record %lld %s", (long long)(bad >> 3), csv::sort_refusal_text(why, b->hdr.n_ref).c_str());
        b->err = buf;
        return finish(CSV_E_INVALID);
    }
    if (record_bytes != inflated - b->hdr.first_rec)
        return finish(fail(b, CSV_E_INVALID, "%scannot sort: the records take %lld bytes, not the stream's", "", (long long)record_bytes));
    // the sorted stream, slice by slice: gathered, compressed, written
    const i64 total = H + record_bytes;
    so.records = n; so.stream = total;
    f = fopen(out_path, "wb");
    if (!f) return finish(fail(b, CSV_E_INVALID, "cannot write %s", out_path));
    i64 coff = 0;
    for (i64 s0 = 0; s0 < total; s0 += slice_bytes) {
        const i64 len = std::min(slice_bytes, total - s0);
        const int32_t nb = (int32_t)((len + csv::SORT_BLOCK - 1) / csv::SORT_BLOCK);
        int64_t out_bytes = 0;
        if (ctx) {
            if ((rc = csv_sort_slice(ctx, s0, len, image.data(), (int64_t)image.size(), sizes.data(), &out_bytes)) != CSV_OK) return finish(fail_sort_device(b, ctx, rc));
        } else {
            csv::sort_tile_fill(slice_h.data(), s0, s0 + len, hdr.data(), H, arena_h.data(), starts.data(), perm.data(), dst.data(), n);
            std::vector<int64_t> off((size_t)nb);
            std::vector<int32_t> ln((size_t)nb);
            for (int32_t k = 0; k < nb; k++) { off[(size_t)k] = (i64)k * csv::SORT_BLOCK; ln[(size_t)k] = (int32_t)std::min<i64>(csv::SORT_BLOCK, len - (i64)k * csv::SORT_BLOCK); }
            rc = csv_bgzf_deflate_host(slice_h.data(), len, nb, off.data(), ln.data(), image.data(), (int64_t)image.size(), sizes.data(), &out_bytes, nullptr);
            if (rc) return finish(fail(b, rc, "%scannot sort: the slice at stream byte %lld does not deflate", "", (long long)s0));
        }
        if (out_bytes <= 0 || out_bytes > (int64_t)image.size()) return finish(fail(b, CSV_E_INVALID, "%scannot sort: the slice at stream byte %lld compressed to nothing", "", (long long)s0));
        if (fwrite(image.data(), 1, (size_t)out_bytes, f) != (size_t)out_bytes) return finish(fail(b, CSV_E_INVALID, "cannot write %s", out_path));
        for (int32_t k = 0; k < nb; k++) {
            so.uoff.push_back(s0 + (i64)k * csv::SORT_BLOCK); so.coff.push_back(coff);
            so.isize.push_back((uint32_t)std::min<i64>(csv::SORT_BLOCK, len - (i64)k * csv::SORT_BLOCK));
            coff += sizes[(size_t)k];
        }
        so.slices++;
    }
    static const uint8_t eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (fwrite(eof_block, 1, sizeof eof_block, f) != sizeof eof_block) return finish(fail(b, CSV_E_INVALID, "cannot write %s", out_path));
    so.uoff.push_back(total); so.coff.push_back(coff); so.isize.push_back(0);
    so.blocks = (i64)so.uoff.size(); so.out_bytes = coff + (i64)sizeof eof_block;
    if (ctx) {
        int64_t up = 0, down = 0;
        csv_sort_counters(ctx, so.ms, &up, &down);
        so.up = up; so.down = down;
        if (b->fr.ctx) {
            int64_t dn_f = 0, up_f = 0;
            csv_frame_counters(b->fr.ctx, nullptr, nullptr, nullptr, &dn_f, &up_f, 0);
            so.up += up_f; so.down += dn_f;
        }
    }
    return finish(CSV_OK);
}

}  // namespace

// ---- the C entry points (include/cutesv_hip.h)
extern "C" {

int csv_bam_struct_size(int which)
{
    switch (which) {
    case 0: return (int)sizeof(csv_bam_chunk);
    case 1: return (int)sizeof(csv_bam_in);
    case 2: return (int)sizeof(csv_bam_out);
    default: return -1;
    }
}

int csv_bam_open(const char* path, int threads, csv_bam** out, char* err, int err_cap)
{
    if (!path || !out) return CSV_E_INVALID;
    *out = nullptr;
    csv_bam* b = new csv_bam;
    csv_bam::File& f = b->file;
    f.threads = std::max(1, std::min(threads, 64));
    f.path = path;
    int rc = CSV_OK;
    struct stat st;
    f.fd = open(path, O_RDONLY);
    if (f.fd < 0 || fstat(f.fd, &st) != 0) rc = fail(b, CSV_E_INVALID, "cannot open %s", path);
    else if (st.st_size < 28) rc = fail(b, CSV_E_INVALID, "%s is too short to be a BAM file (truncated?)", path);
    else {
        f.size = st.st_size;
        void* m = mmap(nullptr, (size_t)f.size, PROT_READ, MAP_PRIVATE, f.fd, 0);
        if (m == MAP_FAILED) rc = fail(b, CSV_E_NOMEM, "cannot map %s", path);
        else f.map = (const uint8_t*)m;
    }
    if (!rc) rc = index_blocks(b);
    if (!rc) rc = read_header(b);
    if (rc) {
        if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", b->err.c_str());
        csv_bam_close(b);
        return rc;
    }
    *out = b;
    return CSV_OK;
}

void csv_bam_close(csv_bam* b)
{
    if (!b) return;
    if (b->file.map) munmap(const_cast<uint8_t*>(b->file.map), (size_t)b->file.size);
    if (b->file.fd >= 0) close(b->file.fd);
    if (b->dev.pin) csv_host_free(b->dev.pin);
    delete b;
}

const char* csv_bam_error(const csv_bam* b) { return b ? b->err.c_str() : ""; }

int csv_bam_header(const csv_bam* b, int32_t* n_ref, const char** names, const int64_t** lengths, const char** text, int64_t* text_len)
{
    if (!b) return CSV_E_INVALID;
    if (n_ref) *n_ref = b->hdr.n_ref;
    if (names) *names = b->hdr.names.data();
    if (lengths) *lengths = b->hdr.lengths.data();
    if (text) *text = b->hdr.text.data();
    if (text_len) *text_len = (int64_t)b->hdr.text.size();
    return CSV_OK;
}

int csv_bam_set_inflate(csv_bam* b, csv_ctx* ctx, int32_t window_blocks)
{
    if (!b || window_blocks > MAX_WINDOW_BLOCKS) return CSV_E_INVALID;
    b->win.n = 0;                                            // the next read fills its window on this route (what open inflated for the header is not kept)
    if (b->fr.ctx) csv_bam_set_frame(b, nullptr);            // (the framing route belongs to the inflate route it was set on)
    b->dev.ctx = ctx;
    b->dev.window_blocks = window_blocks > 0 ? window_blocks : CSV_BAM_WINDOW_BLOCKS;
    return CSV_OK;
}

int csv_bam_set_frame(csv_bam* b, csv_ctx* ctx)
{
    if (!b) return CSV_E_INVALID;
    if (ctx && b->dev.ctx != ctx) return fail(b, CSV_E_STATE, "%sframing on the device needs the device inflate route on the same context (csv_bam_set_inflate)", "");
    if (b->fr.ctx) csv_frame_reader(b->fr.ctx, b, 0);
    if (ctx && csv_frame_reader(ctx, b, 1) != CSV_OK) {
        b->fr.ctx = nullptr; b->win.n = 0;
        return fail(b, CSV_E_STATE, "%sanother reader frames on this context: one framing reader per context (csv_bam_set_frame(other, NULL) first)", "");
    }
    b->fr.ctx = ctx;
    b->win.n = 0; b->fr.valid = false; b->fr.chunk = false; b->fr.pending.clear();
    return CSV_OK;
}

int csv_bam_inflate_stats(const csv_bam* b, int64_t* device_blocks, int64_t* fallback_blocks, double* ms_kernels)
{
    if (!b) return CSV_E_INVALID;
    if (device_blocks) *device_blocks = b->dev.device_blocks;
    if (fallback_blocks) *fallback_blocks = b->dev.fallback_blocks;
    if (ms_kernels) *ms_kernels = b->dev.ms_kernels;
    return CSV_OK;
}

int csv_bam_frame_stats(const csv_bam* b, int64_t* right_blocks, int64_t* fallback_blocks, double* ms_kernels, int64_t* bytes_down, int64_t* bytes_up)
{
    if (!b) return CSV_E_INVALID;
    if (right_blocks) *right_blocks = 0;
    if (fallback_blocks) *fallback_blocks = 0;
    if (ms_kernels) *ms_kernels = 0;
    if (bytes_down) *bytes_down = 0;
    if (bytes_up) *bytes_up = 0;
    if (!b->fr.ctx) return CSV_OK;
    return csv_frame_counters(b->fr.ctx, right_blocks, fallback_blocks, ms_kernels, bytes_down, bytes_up, 0);
}

int csv_bam_read(csv_bam* b, int32_t refid, int64_t beg, int64_t end, int64_t max_records, int32_t flags, csv_bam_chunk* out)
{
    if (!b || !out || max_records < 1) return CSV_E_INVALID;
    b->scan.range_i = 0;
    return read_ranges(b, refid, 1, &beg, &end, max_records, flags, out);
}

int csv_bam_read_ranges(csv_bam* b, int32_t refid, int32_t n_ranges, const int64_t* beg, const int64_t* end, int64_t max_records, int32_t flags, csv_bam_chunk* out)
{
    if (!b || !out || max_records < 1 || n_ranges < 1 || !beg || !end) return CSV_E_INVALID;
    for (int32_t i = 0; i < n_ranges; i++)
        if (beg[i] > end[i] || (i && beg[i] < end[i - 1])) return fail(b, CSV_E_INVALID, "%sthe ranges of a read must be sorted and disjoint (range %lld)", "", i);
    return read_ranges(b, refid, (size_t)n_ranges, beg, end, max_records, flags, out);
}

int csv_bam_chunk_lengths(const csv_bam* b, int32_t* l_read_name, int32_t* l_seq)
{
    if (!b) return CSV_E_INVALID;
    const size_t n = b->chunk.rec_off.size();
    for (size_t i = 0; i < n; i++) {
        if (b->fr.chunk) {
            if (l_read_name) l_read_name[i] = b->fr.l_name_v[i];
            if (l_seq) l_seq[i] = b->fr.l_seq_v[i];
        } else {
            const uint8_t* p = b->chunk.slim.data() + b->chunk.rec_off[i];
            if (l_read_name) l_read_name[i] = p[8];
            if (l_seq) l_seq[i] = (int32_t)rd_u32(p + 16);
        }
    }
    return CSV_OK;
}

int csv_bam_chunk_fetch(csv_bam* b, uint8_t* slim, uint8_t* host)
{
    if (!b) return CSV_E_INVALID;
    if (!b->fr.ctx || !b->fr.chunk) return fail(b, CSV_E_STATE, "%sthe reader holds no device chunk (csv_bam_set_frame; it lives until the next read or route change)", "");
    const int rc = csv_frame_fetch(b->fr.ctx, b, slim, host);
    if (rc) return fail(b, rc, "the device chunk cannot be fetched: %s", csv_last_error(b->fr.ctx));
    return CSV_OK;
}

int csv_bam_index_load(csv_bam* b, const char* path)
{
    if (!b) return CSV_E_INVALID;
    const std::string& bam = b->file.path;
    std::vector<std::string> tries;
    if (path) tries.push_back(path);
    else {
        tries.push_back(bam + ".bai");
        const bool stem = bam.size() > 4 && bam.compare(bam.size() - 4, 4, ".bam") == 0;
        if (stem) tries.push_back(bam.substr(0, bam.size() - 4) + ".bai");
        tries.push_back(bam + ".csi");
        if (stem) tries.push_back(bam.substr(0, bam.size() - 4) + ".csi");
    }
    for (const std::string& t : tries) {
        std::vector<uint8_t> data;
        if (!read_file(t, &data)) continue;
        bai::Index ix;
        csi::Index cx;
        std::vector<uint8_t> payload;
        std::string err;
        const bool is_csi = looks_like_bgzf(data);            // the format is told by content, never by the file's name
        const bool ok = is_csi ? inflate_index_file(data, t, &payload, &err) && csi::parse(payload.data(), payload.size(), b->hdr.n_ref, t.c_str(), voff_check, b, &cx, &err)
                               : bai::parse(data.data(), data.size(), b->hdr.n_ref, t.c_str(), voff_check, b, &ix, &err);
        if (!ok) {
            csv_bam_index_drop(b);                           // a reader whose load failed has no index, whatever it had
            b->err = err;
            return CSV_E_INVALID;
        }
        if (is_csi) install_index(b, std::move(cx), nullptr, nullptr); else install_index(b, std::move(ix), nullptr);
        return CSV_OK;
    }
    b->err = path ? std::string("cannot read the index ") + path : "no index beside " + bam + " (" + tries[0] + (tries.size() > 1 ? ", " + tries[1] : "") + ")";
    return CSV_E_STATE;
}

int csv_bam_index_drop(csv_bam* b)
{
    if (!b) return CSV_E_INVALID;
    b->ix.index = bai::Index(); b->ix.csi = csi::Index();
    b->ix.format = CSV_BAM_INDEX_NONE;
    b->ix.n_mapped.clear(); b->ix.n_unmapped.clear(); b->ix.has_no_coor = false;
    b->ix.has = b->ix.built = false; b->ix.bytes.clear(); b->ix.payload.clear();
    b->scan.hint_at = -1; b->scan.ahead_block = -1; b->scan.seeked = false;
    return CSV_OK;
}

int csv_bam_index_stats(const csv_bam* b, int64_t* mapped, int64_t* unmapped, int64_t* n_no_coor)
{
    if (!b) return CSV_E_INVALID;
    if (!b->ix.has) return CSV_E_STATE;
    for (int32_t r = 0; r < b->hdr.n_ref; r++) {
        if (mapped) mapped[r] = (int64_t)b->ix.n_mapped[(size_t)r];
        if (unmapped) unmapped[r] = (int64_t)b->ix.n_unmapped[(size_t)r];
    }
    if (n_no_coor) *n_no_coor = b->ix.has_no_coor ? (int64_t)b->ix.n_no_coor : -1;
    return CSV_OK;
}

int64_t csv_bam_index_block(const csv_bam* b, int32_t refid, int64_t beg)
{
    if (!b || !b->ix.has || refid < 0 || refid >= b->hdr.n_ref) return -2;
    uint64_t v;
    if (!index_start(b->ix, refid, beg, &v)) return -1;
    if ((v >> 16) == (uint64_t)b->file.size) return (int64_t)b->file.blocks.size() - 1;
    size_t k;
    stream_offset(b, v, &k);
    return (int64_t)k;
}

int csv_bam_index_format(const csv_bam* b) { return b && b->ix.has ? b->ix.format : CSV_BAM_INDEX_NONE; }

// the build of either format: csi NULL - a .bai
static int index_build(csv_bam* b, const csv::IxFormat* csi, int64_t* n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    csv_bam::Index& x = b->ix;
    csv_bam::Scan& s = b->scan;
    begin_read(b);                                           // the build is a read; the scan state of a region is forgotten as well
    s.seeked = false; s.ahead_block = -1; s.hint_at = -1; s.range_i = 0;
    x.records = x.runs = x.frame_runs = x.windows = x.up = x.down = x.bins = 0; x.ms_kernels = x.ms_loff = 0;
    IxTables T;
    for (const Block& k : b->file.blocks) { T.uoff.push_back(k.uoff); T.coff.push_back(k.coff); T.isize.push_back(k.isize); }
    T.l_ref.assign(b->hdr.lengths.begin(), b->hdr.lengths.end());
    csv::ix::Builder B;
    B.begin(b->hdr.n_ref, T.l_ref.data(), csi ? *csi : csv::ix_bai(), csi != nullptr);
    s.cur = b->hdr.first_rec;
    const int rc = b->fr.ctx ? index_build_device(b, T, &B) : index_build_host(b, T, &B);
    x.ms_kernels = b->dev.ms_kernels;
    if (b->fr.ctx) {
        double ms_f = 0, ms_x = 0;
        int64_t dn_f = 0, up_f = 0, dn_x = 0, up_x = 0, wins = 0;
        csv_frame_counters(b->fr.ctx, nullptr, nullptr, &ms_f, &dn_f, &up_f, 0);
        csv_index_counters(b->fr.ctx, &ms_x, &dn_x, &up_x, &wins);
        x.ms_kernels += ms_f + ms_x; x.down = dn_f + dn_x; x.up = up_f + up_x; x.windows = wins;
    }
    s.cur = b->hdr.first_rec;
    b->win.n = 0; b->fr.valid = false;                       // (what a later read costs does not depend on what the build left in the window)
    if (rc) return rc;
    x.records = B.records;
    if (!b->fr.ctx) x.runs = (i64)B.runs.size();
    // the built bytes take the path a file's bytes take: parsed and validated against this file's blocks, then installed
    if (csi) {
        x.bins = (i64)B.pairs().size() / 2;
        if (b->fr.ctx && csv_index_loff_ms) x.ms_loff = csv_index_loff_ms(b->fr.ctx);
        std::vector<uint8_t> payload = B.bytes_csi(), bytes;
        csi::Index cx;
        std::string err;
        if (!csi::parse(payload.data(), payload.size(), b->hdr.n_ref, "the built index", voff_check, b, &cx, &err)) {
            b->err = "cannot build the index: " + err;
            return CSV_E_INVALID;
        }
        if (!bgzf_compress(payload, &bytes)) return fail(b, CSV_E_INVALID, "%scannot build the index: the payload does not deflate", "");
        install_index(b, std::move(cx), &bytes, &payload);
        if (n_bytes) *n_bytes = (int64_t)x.bytes.size();
        return CSV_OK;
    }
    std::vector<uint8_t> bytes = B.bytes();
    bai::Index ix;
    std::string err;
    if (!bai::parse(bytes.data(), bytes.size(), b->hdr.n_ref, "the built index", voff_check, b, &ix, &err)) {
        b->err = "cannot build the index: " + err;
        return CSV_E_INVALID;
    }
    install_index(b, std::move(ix), &bytes);
    if (n_bytes) *n_bytes = (int64_t)x.bytes.size();
    return CSV_OK;
}

int csv_bam_index_build(csv_bam* b, int32_t flags, int64_t* n_bytes)
{
    if (!b || flags != 0) return CSV_E_INVALID;
    return index_build(b, nullptr, n_bytes);
}

int csv_bam_index_build_csi(csv_bam* b, int32_t min_shift, int32_t depth, int64_t* n_bytes)
{
    if (!b) return CSV_E_INVALID;
    if (n_bytes) *n_bytes = 0;
    if (min_shift < 4 || min_shift > 31 || depth < 0) return fail(b, CSV_E_INVALID, "%scannot build the index: min_shift must be 4 .. 31 and depth 0 or more (min_shift %lld)", "", min_shift);
    const std::vector<csv::ix_i64> l_ref(b->hdr.lengths.begin(), b->hdr.lengths.end());
    if (depth == 0) depth = csv::ix::auto_depth(min_shift, b->hdr.n_ref, l_ref.data());
    const csv::IxFormat F = csv::ix_format(min_shift, depth);
    if (!csv::ix_format_ok(F)) return fail(b, CSV_E_INVALID, "%scannot build the index: min_shift + 3 * depth must stay at or below 62 and depth at or below 9 (depth %lld)", "", depth);
    csv::ix_i64 entries = 0;
    for (i64 l : b->hdr.lengths) entries += csv::ix_lin_entries(l, F);
    if (entries > MAX_LIN_ENTRIES) return fail(b, CSV_E_INVALID, "%scannot build the index: min_shift is too small for these references (%lld windows)", "", (long long)entries);
    return index_build(b, &F, n_bytes);
}

int csv_bam_index_payload(const csv_bam* b, uint8_t* out, int64_t cap, int64_t* need)
{
    if (!b) return CSV_E_INVALID;
    if (need) *need = 0;
    if (!b->ix.has || !b->ix.built || b->ix.format != CSV_BAM_INDEX_CSI) return CSV_E_STATE;
    if (need) *need = (int64_t)b->ix.payload.size();
    if (!out || cap < (int64_t)b->ix.payload.size()) return CSV_E_CAPACITY;
    memcpy(out, b->ix.payload.data(), b->ix.payload.size());
    return CSV_OK;
}

int csv_bam_index_build_stats_csi(const csv_bam* b, int64_t* bins, double* ms_loff)
{
    if (!b) return CSV_E_INVALID;
    if (bins) *bins = b->ix.bins;
    if (ms_loff) *ms_loff = b->ix.ms_loff;
    return CSV_OK;
}

int csv_bam_index_bytes(const csv_bam* b, uint8_t* out, int64_t cap, int64_t* need)
{
    if (!b) return CSV_E_INVALID;
    if (need) *need = 0;
    if (!b->ix.has || !b->ix.built) return CSV_E_STATE;
    if (need) *need = (int64_t)b->ix.bytes.size();
    if (!out || cap < (int64_t)b->ix.bytes.size()) return CSV_E_CAPACITY;
    memcpy(out, b->ix.bytes.data(), b->ix.bytes.size());
    return CSV_OK;
}

int csv_bam_index_build_stats(const csv_bam* b, int64_t* records, int64_t* runs, double* ms_kernels, int64_t* bytes_up, int64_t* bytes_down, int64_t* frame_runs,
                              int64_t* index_windows)
{
    if (!b) return CSV_E_INVALID;
    if (records) *records = b->ix.records;
    if (runs) *runs = b->ix.runs;
    if (ms_kernels) *ms_kernels = b->ix.ms_kernels;
    if (bytes_up) *bytes_up = b->ix.up;
    if (bytes_down) *bytes_down = b->ix.down;
    if (frame_runs) *frame_runs = b->ix.frame_runs;
    if (index_windows) *index_windows = b->ix.windows;
    return CSV_OK;
}

int csv_bam_sort(csv_bam* b, csv_ctx* ctx, const char* out_path, int64_t max_bytes, int32_t slice_blocks, int32_t flags)
{
    if (!b) return CSV_E_INVALID;
    if (!ctx || !out_path || flags != 0 || slice_blocks < 0 || slice_blocks > 32768) return fail(b, CSV_E_INVALID, "%sbad sort call", "");
    if (b->dev.ctx && b->dev.ctx != ctx) return fail(b, CSV_E_STATE, "%sthe sort needs the context the reader inflates on", "");
    return sort_run(b, ctx, out_path, max_bytes, slice_blocks);
}

int csv_bam_sort_host(csv_bam* b, const char* out_path, int64_t max_bytes, int32_t slice_blocks, int32_t flags)
{
    if (!b) return CSV_E_INVALID;
    if (!out_path || flags != 0 || slice_blocks < 0 || slice_blocks > 32768) return fail(b, CSV_E_INVALID, "%sbad sort call", "");
    if (b->fr.ctx) return fail(b, CSV_E_STATE, "%sthe host form of the sort frames on the host (csv_bam_set_frame(bam, NULL) first)", "");
    return sort_run(b, nullptr, out_path, max_bytes, slice_blocks);
}

int csv_bam_sort_stats(const csv_bam* b, int64_t* counts, double* ms)
{
    if (!b) return CSV_E_INVALID;
    const csv_bam::Sorted& so = b->so;
    if (counts) { const int64_t v[10] = {so.records, so.inversions, so.inflated, so.stream, so.out_bytes, so.blocks, so.slices, so.passes, so.up, so.down}; memcpy(counts, v, sizeof v); }
    if (ms) memcpy(ms, so.ms, sizeof so.ms);
    return CSV_OK;
}

int csv_bam_sort_blocks(const csv_bam* b, int64_t* uoff, int64_t* coff, uint32_t* isize, int64_t cap, int64_t* need)
{
    if (!b) return CSV_E_INVALID;
    const csv_bam::Sorted& so = b->so;
    const int64_t n = (int64_t)so.uoff.size();
    if (need) *need = n;
    if (n == 0) return CSV_E_STATE;
    if (!uoff || !coff || !isize || cap < n) return CSV_E_CAPACITY;
    for (int64_t k = 0; k < n; k++) { uoff[k] = so.uoff[(size_t)k]; coff[k] = so.coff[(size_t)k]; isize[k] = so.isize[(size_t)k]; }
    return CSV_OK;
}

}  // extern "C"
