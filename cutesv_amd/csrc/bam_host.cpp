// bam_host.cpp — the host side of the native BAM reader: BGZF inflate on host threads, the BAM
// header, record framing, region scan and the slim image the decode kernels (bam.hip.h) take.  With csv_bam_set_inflate the
// windows are inflated on the device instead (csv_bgzf_inflate) and the host inflates only the blocks
// the device gave up on.
//
// Written from the SAM/BAM specification (SAMv1, sections 4.1 "The BGZF compression format" and 4.2 "The BAM format"):
//   BGZF block  = gzip member with one extra subfield 'B','C' (u16 BSIZE = block size - 1), raw deflate payload, CRC32, ISIZE
//   BAM         = "BAM\1", l_text, text, n_ref, {l_name, name, l_ref} * n_ref, then records
//   record      = block_size, then block_size bytes: refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID
//                 next_pos tlen (32 bytes), read_name, cigar (u32 * n_cigar_op), seq ((l_seq + 1) / 2), qual (l_seq), aux
// Without an index a region is a forward scan over the sorted records with an early exit.  With one (csv_bam_index_load,
// bai_index.h) the scan starts at the linear-index entry of the region's first window; the index moves the
// starting point and nothing else.  What goes to the device per
// record is the slim image {32 fixed bytes, CIGAR words, aux bytes}; the read name and the 4-bit sequence stay in a host
// buffer; the qualities are dropped.
// csv_bam_index_build makes the index a file came without: one whole-file pass on the reader's current routes,
// through index_core.h - a host loop over the records, or, on the framing route, the index kernels over the rows of every window.
// With csv_bam_set_frame the window never leaves the device: the records are framed there (frame_core.h), the
// selection loop below runs over the rows of the record table instead of the bytes, and the two images are built in device memory.
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
#include <string>
#include <thread>
#include <vector>

#include "../../include/cutesv_hip.h"
#include "bai_index.h"
#include "frame_core.h"
#include "index_core.h"

namespace {

typedef int64_t i64;

inline uint32_t rd_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }     // (little-endian hosts only, as the rest of the library)
inline int32_t  rd_i32(const uint8_t* p) { int32_t v; memcpy(&v, p, 4); return v; }
inline uint16_t rd_u16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Block { i64 coff; int32_t csize, hdr; uint32_t isize; i64 uoff; };      // coff: file offset, hdr: bytes before the deflate payload

constexpr i64 SLIM_ALIGN = 16;               // a slim record starts 16-byte aligned: its CIGAR words (at + 32) are too
constexpr int REFILL_BLOCKS = 256;           // BGZF blocks inflated per refill of the window (<= 16 MiB inflated)
constexpr int AHEAD_STEP_BLOCKS = 16;        // ... past the guessed end of an indexed region
constexpr int MAX_WINDOW_BLOCKS = 16384;     // ... on the device route at most (csv_bam_set_inflate; <= 1 GiB inflated)

}  // namespace

struct csv_bam {
    int            fd = -1;
    const uint8_t* map = nullptr;
    i64            fsize = 0;
    std::string    path;
    int            threads = 1;
    std::string    err;
    std::vector<Block> blocks;
    i64            utotal = 0;
    // header
    std::string          text, names;       // names: NUL-terminated, back to back
    std::vector<i64>     lengths;
    int32_t              n_ref = 0;
    i64                  first_rec = 0;      // uncompressed offset of the first record
    // the inflated window [win_u0, win_u0 + win.size())
    std::vector<uint8_t> win;                // (the host route's storage)
    const uint8_t*       win_p = nullptr;    // the window's bytes: win.data(), or the page-locked window of the device route
    i64                  win_n = 0;
    i64                  win_u0 = 0;
    size_t               win_b1 = 0;         // the window holds the blocks up to this one (exclusive)
    // the device route (csv_bam_set_inflate): the context, blocks per window, the page-locked window, the tables of one call
    csv_ctx*             dev = nullptr;
    int                  window_blocks = REFILL_BLOCKS;
    uint8_t*             pin = nullptr;
    i64                  pin_cap = 0;
    std::vector<int64_t> d_in_off, d_out_off;
    std::vector<int32_t> d_in_len, d_out_len;
    std::vector<uint32_t> d_crc;
    std::vector<uint8_t> d_status;
    i64                  device_blocks = 0, fallback_blocks = 0;
    double               ms_kernels = 0;
    i64                  cur = 0;            // uncompressed offset of the next record
    std::map<uint32_t, i64> contig_at;       // (uint32)refID -> offset of its first record, as found (-1 sorts last, as in a sorted file)
    uint32_t             scanned_key = 0;    // every contig with a key <= this one that exists is in contig_at
    bool                 scanned_any = false;
    // the last region scan: its first record.  Records before it end at or before hint_beg, so a later region of the same
    // contig that begins at or after hint_beg starts its scan there
    uint32_t             hint_key = 0;
    i64                  hint_beg = 0, hint_at = -1;
    // the index (csv_bam_index_load): the scan of a region starts at its linear-index entry.  seek_key: the contig the running scan
    // was positioned in by the index - the first record it sees of that contig is not the contig's first
    bool                 has_index = false;
    bai::Index           index;
    // a built index (csv_bam_index_build): its bytes, as a .bai file holds them, and the counters of the build
    bool                 index_built = false;
    std::vector<uint8_t> index_bytes;
    i64                  ix_records = 0, ix_runs = 0, ix_frame_runs = 0, ix_windows = 0, ix_up = 0, ix_down = 0;
    double               ix_ms_kernels = 0;
    bool                 seeked = false;
    uint32_t             seek_key = 0;
    i64                  ahead_block = -1;   // with an index: the block where the running region is guessed to end (-1: no guess)
    size_t               range_i = 0;        // csv_bam_read_ranges: the range the scan is in
    // the chunk handed out last
    std::vector<uint8_t> slim, host;
    std::vector<i64>     rec_off, host_off;
    std::vector<uint32_t> rec_len;
    double               ms_inflate = 0;
    i64                  inflated = 0, compressed = 0;
    // the framing route (csv_bam_set_frame): the window lies in the context's device memory and is known here by its rows - the
    // records the chain from fr_from met, up to fr_tail where it stopped (stream offsets).  pending: the selected records of the
    // current window that are not packed yet; slim_size / host_size: the bytes of the device images with them
    csv_ctx*             frame = nullptr;
    uint64_t             fr_serial = 0;
    size_t               win_b0 = 0;
    const csv::FrRow*    fr_rows = nullptr;
    i64                  fr_n = 0, fr_i = 0, fr_from = 0, fr_tail = 0;
    int32_t              fr_tail_bs = 0;
    bool                 fr_tail_has_bs = false, fr_valid = false, framed_chunk = false;
    std::vector<csv::FrPack> pending;
    std::vector<int32_t> l_name_v, l_seq_v, t_len;
    std::vector<int64_t> t_off;
    std::vector<uint8_t> one_block;
    i64                  slim_size = 0, host_size = 0;
};

namespace {

int fail(csv_bam* b, int code, const char* fmt, const char* a = "", long long x = 0)
{
    char buf[512];
    snprintf(buf, sizeof buf, fmt, a, x);
    b->err = buf;
    return code;
}

// the block table: one pass over the block headers of the mapped file
int index_blocks(csv_bam* b)
{
    i64 o = 0, u = 0;
    while (o < b->fsize) {
        const uint8_t* p = b->map + o;
        if (o + 18 > b->fsize) return fail(b, CSV_E_INVALID, "%struncated BGZF block header at byte %lld", "", (long long)o);
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return fail(b, CSV_E_INVALID, "%snot a BGZF block at byte %lld", "", (long long)o);
        const int xlen = rd_u16(p + 10);
        if (o + 12 + xlen > b->fsize) return fail(b, CSV_E_INVALID, "%struncated BGZF block header at byte %lld", "", (long long)o);
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
        if (o + total > b->fsize) return fail(b, CSV_E_INVALID, "%struncated BGZF block at byte %lld", "", (long long)o);
        Block k;
        k.coff = o; k.csize = (int32_t)total; k.hdr = 12 + xlen; k.isize = rd_u32(p + total - 4); k.uoff = u;
        if (k.isize > 65536) return fail(b, CSV_E_INVALID, "%sBGZF block inflates to more than 64 KiB at byte %lld", "", (long long)o);
        b->blocks.push_back(k);
        u += k.isize; o += total;
    }
    b->utotal = u;
    if (b->blocks.empty() || b->blocks.back().isize != 0 || b->blocks.back().csize != 28)
        return fail(b, CSV_E_INVALID, "%sthe BGZF end-of-file block is missing (truncated file?)", "");
    return CSV_OK;
}

bool inflate_block(const csv_bam* b, const Block& k, uint8_t* dst)
{
    if (k.isize == 0) return true;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = const_cast<Bytef*>(b->map + k.coff + k.hdr);
    z.avail_in = (uInt)(k.csize - k.hdr - 8);
    z.next_out = dst; z.avail_out = k.isize;
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.avail_out == 0;
    inflateEnd(&z);
    if (!ok) return false;
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, k.isize) == rd_u32(b->map + k.coff + k.csize - 8);
}

// the window becomes the inflated blocks [b0, b1), on the device: the mapped file from the first block's header to the last
// block's trailer is the `comp` of one csv_bgzf_inflate (the payloads lie in it where they are: nothing is gathered), the bytes land
// in the page-locked window, and every block the device reports is inflated again by inflate_block, whose verdict stands
int load_window_device(csv_bam* b, size_t b0, size_t b1, size_t bn, i64 keep)
{
    const double t0 = now_ms();
    const i64 keep_at = b->blocks[b0].uoff - b->win_u0;      // (only with keep > 0: where the kept bytes lie in the old window)
    b->win_n = 0;
    const i64 bytes = (b1 < b->blocks.size() ? b->blocks[b1].uoff : b->utotal) - b->blocks[b0].uoff;
    if (bytes > b->pin_cap) {
        void* p = nullptr;
        const i64 want = bytes + bytes / 4 + 4096;
        if (csv_host_alloc(want, &p) != CSV_OK) return fail(b, CSV_E_NOMEM, "%scannot page-lock an inflate window of %lld bytes", "", (long long)want);
        if (keep > 0) memcpy(p, b->pin + keep_at, (size_t)keep);
        if (b->pin) csv_host_free(b->pin);
        b->pin = (uint8_t*)p; b->pin_cap = want;
    } else if (keep > 0 && keep_at > 0) memmove(b->pin, b->pin + keep_at, (size_t)keep);
    b->win_u0 = b->blocks[b0].uoff;
    b0 = bn;                                                 // the blocks in front of bn are the kept bytes: inflated already
    const size_t n = b1 - b0;
    b->d_in_off.resize(n); b->d_in_len.resize(n); b->d_out_off.resize(n); b->d_out_len.resize(n); b->d_crc.resize(n); b->d_status.resize(n);
    const i64 base = b->blocks[b0].coff, comp_bytes = b->blocks[b1 - 1].coff + b->blocks[b1 - 1].csize - base;
    for (size_t j = 0; j < n; j++) {
        const Block& k = b->blocks[b0 + j];
        b->d_in_off[j] = k.coff + k.hdr - base; b->d_in_len[j] = k.csize - k.hdr - 8;
        b->d_out_off[j] = k.uoff - b->win_u0; b->d_out_len[j] = (int32_t)k.isize;
        b->d_crc[j] = rd_u32(b->map + k.coff + k.csize - 8);
    }
    double ms = 0;
    const int rc = n == 0 ? CSV_OK : csv_bgzf_inflate(b->dev, b->map + base, comp_bytes, (int32_t)n, b->d_in_off.data(), b->d_in_len.data(), b->d_out_off.data(), b->d_out_len.data(),
                                    b->d_crc.data(), b->pin, bytes, 0, b->d_status.data(), &ms);
    if (rc) return fail(b, rc, "the device inflate failed: %s", csv_last_error(b->dev));
    b->ms_kernels += ms;
    i64 bad = -1;
    for (size_t j = 0; j < n; j++) {
        if (!b->d_status[j]) { b->device_blocks++; continue; }
        b->fallback_blocks++;
        if (!inflate_block(b, b->blocks[b0 + j], b->pin + b->d_out_off[j])) bad = (i64)(b0 + j);
    }
    for (size_t j = b0; j < b1; j++) b->compressed += b->blocks[j].csize;
    b->inflated += bytes - keep;
    b->ms_inflate += now_ms() - t0;
    if (bad >= 0) return fail(b, CSV_E_INVALID, "%sBGZF block at byte %lld does not inflate (or fails its CRC)", "", (long long)b->blocks[(size_t)bad].coff);
    b->win_p = b->pin; b->win_n = bytes; b->win_b1 = b1;
    return CSV_OK;
}

int frame_flush(csv_bam* b)
{
    if (b->pending.empty()) return CSV_OK;
    const int rc = csv_frame_pack(b->frame, (int64_t)b->pending.size(), b->pending.data(), b->slim_size, b->host_size);
    b->pending.clear();
    if (rc) return fail(b, rc, "the device framing failed: %s", csv_last_error(b->frame));
    return CSV_OK;
}

// load_window_device for the framing route: the bytes are inflated into the context's device window and stay there; the kept tail
// is carried over on the device; a block the device gives up on is inflated by inflate_block, whose verdict stands, and copied up
int load_window_frame(csv_bam* b, size_t b0, size_t b1, size_t bn, i64 keep)
{
    int rc = frame_flush(b);                                 // (the selected records of the old window are packed out of it first)
    if (rc) return rc;
    const double t0 = now_ms();
    const i64 keep_at = keep > 0 ? b->blocks[b0].uoff - b->win_u0 : 0;
    b->win_n = 0; b->fr_valid = false;
    const i64 u0 = b->blocks[b0].uoff, bytes = (b1 < b->blocks.size() ? b->blocks[b1].uoff : b->utotal) - u0;
    const size_t n = b1 > bn ? b1 - bn : 0;
    b->d_in_off.resize(n); b->d_in_len.resize(n); b->d_out_off.resize(n); b->d_out_len.resize(n); b->d_crc.resize(n); b->d_status.resize(n);
    const i64 base = n ? b->blocks[bn].coff : 0, comp_bytes = n ? b->blocks[b1 - 1].coff + b->blocks[b1 - 1].csize - base : 0;
    for (size_t j = 0; j < n; j++) {
        const Block& k = b->blocks[bn + j];
        b->d_in_off[j] = k.coff + k.hdr - base; b->d_in_len[j] = k.csize - k.hdr - 8;
        b->d_out_off[j] = k.uoff - u0; b->d_out_len[j] = (int32_t)k.isize;
        b->d_crc[j] = rd_u32(b->map + k.coff + k.csize - 8);
    }
    double ms = 0;
    rc = csv_frame_window(b->frame, b->map + base, comp_bytes, (int32_t)n, b->d_in_off.data(), b->d_in_len.data(), b->d_out_off.data(), b->d_out_len.data(), b->d_crc.data(), bytes,
                          keep, keep_at, b->d_status.data(), &ms);
    if (rc) return fail(b, rc, "the device inflate failed: %s", csv_last_error(b->frame));
    b->fr_serial = csv_frame_window_serial(b->frame);
    b->win_u0 = u0;
    b->ms_kernels += ms;
    i64 bad = -1;
    b->one_block.resize(65536);
    for (size_t j = 0; j < n; j++) {
        if (!b->d_status[j]) { b->device_blocks++; continue; }
        b->fallback_blocks++;
        if (!inflate_block(b, b->blocks[bn + j], b->one_block.data())) { bad = (i64)(bn + j); continue; }
        // (the window is not valid to the reader yet, but it is the context's: the block goes where the device would have put it)
        rc = csv_frame_window_put(b->frame, b->d_out_off[j], b->one_block.data(), b->d_out_len[j]);
        if (rc) return fail(b, rc, "the device inflate failed: %s", csv_last_error(b->frame));
    }
    for (size_t j = bn; j < b1; j++) b->compressed += b->blocks[j].csize;
    b->inflated += bytes - keep;
    b->ms_inflate += now_ms() - t0;
    if (bad >= 0) return fail(b, CSV_E_INVALID, "%sBGZF block at byte %lld does not inflate (or fails its CRC)", "", (long long)b->blocks[(size_t)bad].coff);
    b->win_p = nullptr; b->win_n = bytes; b->win_b0 = b0; b->win_b1 = b1;
    return CSV_OK;
}

// the window becomes the inflated blocks [b0, b1).  keep > 0: the window already holds the bytes of the blocks [b0, bn) at its end
// (the scan moved on inside it): they are moved to the front and only [bn, b1) is inflated; else bn == b0
int load_window(csv_bam* b, size_t b0, size_t b1, size_t bn, i64 keep)
{
    if (b->frame) return load_window_frame(b, b0, b1, bn, keep);
    if (b->dev) return load_window_device(b, b0, b1, bn, keep);
    const double t0 = now_ms();
    const i64 bytes = (b1 < b->blocks.size() ? b->blocks[b1].uoff : b->utotal) - b->blocks[b0].uoff;
    if (keep > 0) memmove(b->win.data(), b->win.data() + (b->blocks[b0].uoff - b->win_u0), (size_t)keep);      // (in place: no fresh pages per refill)
    b->win.resize((size_t)bytes);
    b->win_n = 0;
    b->win_u0 = b->blocks[b0].uoff;
    b0 = bn;
    std::atomic<size_t> next(b0);
    std::atomic<i64> bad(-1);
    auto work = [&] {
        for (;;) {
            const size_t k = next.fetch_add(8);            // 8 blocks at a time: neighbours stay on one thread
            if (k >= b1) return;
            for (size_t j = k; j < std::min(k + 8, b1); j++)
                if (!inflate_block(b, b->blocks[j], b->win.data() + (b->blocks[j].uoff - b->win_u0))) bad.store((i64)j);
        }
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)b->threads, (b1 - b0 + 7) / 8));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    for (size_t j = b0; j < b1; j++) b->compressed += b->blocks[j].csize;
    b->inflated += bytes - keep;
    b->ms_inflate += now_ms() - t0;
    if (bad.load() >= 0) return fail(b, CSV_E_INVALID, "%sBGZF block at byte %lld does not inflate (or fails its CRC)", "", (long long)b->blocks[(size_t)bad.load()].coff);
    b->win_p = b->win.data(); b->win_n = bytes; b->win_b1 = b1;
    return CSV_OK;
}

size_t block_of(const csv_bam* b, i64 u)                  // the block that holds uncompressed offset u (u < utotal)
{
    size_t lo = 0, hi = b->blocks.size();
    while (hi - lo > 1) { const size_t m = (lo + hi) / 2; if (b->blocks[m].uoff <= u) lo = m; else hi = m; }
    while (lo + 1 < b->blocks.size() && b->blocks[lo].isize == 0) lo++;
    return lo;
}

// the window holds [u, u + need) of the inflated stream afterwards (refilled when it did not); *have = false: the stream ends
// before u + need
int ensure(csv_bam* b, i64 u, i64 need, bool* have)
{
    *have = false;
    if (u + need > b->utotal) return CSV_OK;
    if (u < b->win_u0 || u + need > b->win_u0 + b->win_n) {
        const size_t b0 = block_of(b, u);
        size_t b1 = std::min(b->blocks.size(), b0 + (size_t)(b->dev ? b->window_blocks : REFILL_BLOCKS));
        if (b->ahead_block >= 0)                             // an indexed region: up to where it is guessed to end, then in small steps
            b1 = std::min(b1, (i64)b0 <= b->ahead_block ? (size_t)b->ahead_block + 1 : b0 + AHEAD_STEP_BLOCKS);
        while (b1 < b->blocks.size() && b->blocks[b1].uoff < u + need) b1++;
        // the scan moved on inside the window: the blocks from b0 to the window's end are there already and are not inflated again
        size_t bn = b0;
        i64 keep = 0;
        if (b->win_n > 0 && u >= b->win_u0 && u < b->win_u0 + b->win_n && b->win_b1 > b0) {
            bn = b->win_b1;
            keep = b->win_u0 + b->win_n - b->blocks[b0].uoff;
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
    return b->win_p + (u - b->win_u0);
}

int read_header(csv_bam* b)
{
    int rc;
    const uint8_t* p = at(b, 0, 12, &rc);
    if (rc) return rc;
    if (!p || memcmp(p, "BAM\1", 4) != 0) return fail(b, CSV_E_INVALID, "%snot a BAM file (no BAM\\1 magic)", "");
    const i64 l_text = rd_i32(p + 4);
    if (l_text < 0) return fail(b, CSV_E_INVALID, "%sbad l_text", "");
    p = at(b, 8, l_text + 4, &rc);
    if (rc) return rc;
    if (!p) return fail(b, CSV_E_INVALID, "%sthe file ends inside the BAM header", "");
    b->text.assign((const char*)p, (size_t)l_text);
    while (!b->text.empty() && b->text.back() == '\0') b->text.pop_back();
    b->n_ref = rd_i32(p + l_text);
    if (b->n_ref < 0) return fail(b, CSV_E_INVALID, "%sbad n_ref", "");
    i64 u = 8 + l_text + 4;
    for (int r = 0; r < b->n_ref; r++) {
        p = at(b, u, 4, &rc);
        if (rc) return rc;
        const i64 l_name = p ? rd_i32(p) : -1;
        if (l_name < 1 || l_name > 1 << 20) return fail(b, CSV_E_INVALID, "%sbad reference name length (reference %lld)", "", r);
        p = at(b, u + 4, l_name + 4, &rc);
        if (rc) return rc;
        if (!p) return fail(b, CSV_E_INVALID, "%sthe file ends inside the BAM header", "");
        b->names.append((const char*)p, strnlen((const char*)p, (size_t)l_name));
        b->names.push_back('\0');
        b->lengths.push_back(rd_u32(p + l_name));
        u += 8 + l_name;
    }
    b->first_rec = b->cur = u;
    return CSV_OK;
}

}  // namespace

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
    b->threads = std::max(1, std::min(threads, 64));
    b->path = path;
    int rc = CSV_OK;
    struct stat st;
    b->fd = open(path, O_RDONLY);
    if (b->fd < 0 || fstat(b->fd, &st) != 0) rc = fail(b, CSV_E_INVALID, "cannot open %s", path);
    else if (st.st_size < 28) rc = fail(b, CSV_E_INVALID, "%s is too short to be a BAM file (truncated?)", path);
    else {
        b->fsize = st.st_size;
        void* m = mmap(nullptr, (size_t)b->fsize, PROT_READ, MAP_PRIVATE, b->fd, 0);
        if (m == MAP_FAILED) rc = fail(b, CSV_E_NOMEM, "cannot map %s", path);
        else b->map = (const uint8_t*)m;
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
    if (b->map) munmap(const_cast<uint8_t*>(b->map), (size_t)b->fsize);
    if (b->fd >= 0) close(b->fd);
    if (b->pin) csv_host_free(b->pin);
    delete b;
}

const char* csv_bam_error(const csv_bam* b) { return b ? b->err.c_str() : ""; }

int csv_bam_header(const csv_bam* b, int32_t* n_ref, const char** names, const int64_t** lengths, const char** text, int64_t* text_len)
{
    if (!b) return CSV_E_INVALID;
    if (n_ref) *n_ref = b->n_ref;
    if (names) *names = b->names.data();
    if (lengths) *lengths = b->lengths.data();
    if (text) *text = b->text.data();
    if (text_len) *text_len = (int64_t)b->text.size();
    return CSV_OK;
}

int csv_bam_set_inflate(csv_bam* b, csv_ctx* ctx, int32_t window_blocks)
{
    if (!b || window_blocks > MAX_WINDOW_BLOCKS) return CSV_E_INVALID;
    b->win_n = 0;                                            // the next read fills its window on this route (what open inflated for the header is not kept)
    if (b->frame) csv_bam_set_frame(b, nullptr);             // (the framing route belongs to the inflate route it was set on)
    b->dev = ctx;
    b->window_blocks = window_blocks > 0 ? window_blocks : CSV_BAM_WINDOW_BLOCKS;
    return CSV_OK;
}

int csv_bam_set_frame(csv_bam* b, csv_ctx* ctx)
{
    if (!b) return CSV_E_INVALID;
    if (ctx && b->dev != ctx) return fail(b, CSV_E_STATE, "%sframing on the device needs the device inflate route on the same context (csv_bam_set_inflate)", "");
    if (b->frame) csv_frame_reader(b->frame, b, 0);
    if (ctx && csv_frame_reader(ctx, b, 1) != CSV_OK) {
        b->frame = nullptr; b->win_n = 0;
        return fail(b, CSV_E_STATE, "%sanother reader frames on this context: one framing reader per context (csv_bam_set_frame(other, NULL) first)", "");
    }
    b->frame = ctx;
    b->win_n = 0; b->fr_valid = false; b->framed_chunk = false; b->pending.clear();
    return CSV_OK;
}

int csv_bam_chunk_lengths(const csv_bam* b, int32_t* l_read_name, int32_t* l_seq)
{
    if (!b) return CSV_E_INVALID;
    const size_t n = b->rec_off.size();
    for (size_t i = 0; i < n; i++) {
        if (b->framed_chunk) {
            if (l_read_name) l_read_name[i] = b->l_name_v[i];
            if (l_seq) l_seq[i] = b->l_seq_v[i];
        } else {
            const uint8_t* p = b->slim.data() + b->rec_off[i];
            if (l_read_name) l_read_name[i] = p[8];
            if (l_seq) l_seq[i] = (int32_t)rd_u32(p + 16);
        }
    }
    return CSV_OK;
}

int csv_bam_chunk_fetch(csv_bam* b, uint8_t* slim, uint8_t* host)
{
    if (!b) return CSV_E_INVALID;
    if (!b->frame || !b->framed_chunk) return fail(b, CSV_E_STATE, "%sthe reader holds no device chunk (csv_bam_set_frame; it lives until the next read or route change)", "");
    const int rc = csv_frame_fetch(b->frame, b, slim, host);
    if (rc) return fail(b, rc, "the device chunk cannot be fetched: %s", csv_last_error(b->frame));
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
    if (!b->frame) return CSV_OK;
    return csv_frame_counters(b->frame, right_blocks, fallback_blocks, ms_kernels, bytes_down, bytes_up, 0);
}

int csv_bam_inflate_stats(const csv_bam* b, int64_t* device_blocks, int64_t* fallback_blocks, double* ms_kernels)
{
    if (!b) return CSV_E_INVALID;
    if (device_blocks) *device_blocks = b->device_blocks;
    if (fallback_blocks) *fallback_blocks = b->fallback_blocks;
    if (ms_kernels) *ms_kernels = b->ms_kernels;
    return CSV_OK;
}

}  // extern "C"

namespace {

// the block a virtual offset of the (validated) index points into -> the offset in the inflated stream
i64 stream_offset(const csv_bam* b, uint64_t voff, size_t* block)
{
    const i64 coff = (i64)(voff >> 16);
    size_t lo = 0, hi = b->blocks.size();
    while (hi - lo > 1) { const size_t m = (lo + hi) / 2; if (b->blocks[m].coff <= coff) lo = m; else hi = m; }
    if (block) *block = lo;
    return b->blocks[lo].uoff + (i64)(voff & 0xffff);
}

int voff_check(void* user, uint64_t voff)
{
    const csv_bam* b = (const csv_bam*)user;
    const i64 coff = (i64)(voff >> 16);
    if (coff == b->fsize) return (voff & 0xffff) ? 2 : 0;     // "behind the last block": where a writer stands after its end-of-file block
    size_t k;
    stream_offset(b, voff, &k);
    if (b->blocks[k].coff != coff) return 1;
    return (voff & 0xffff) > b->blocks[k].isize ? 2 : 0;
}

// the index positions the scan for range [beg, end) of contig `key`: the cursor moves forward only (never behind `floor`);
// -> false: the index says that no record overlaps any window from beg's on
bool index_seek(csv_bam* b, uint32_t key, i64 beg, i64 end, i64 floor)
{
    uint64_t v;
    if (!bai::start_offset(b->index, (int32_t)key, beg, &v)) return false;
    const i64 u = (v >> 16) == (uint64_t)b->fsize ? b->utotal : stream_offset(b, v, nullptr);
    b->cur = u > floor ? u : floor;
    b->seeked = true; b->seek_key = key;                     // (also from `floor`, a hint: the scan that set it was positioned by the index too)
    size_t k = b->blocks.size() - 1;
    if (bai::stop_guess(b->index, (int32_t)key, end, &v) && (v >> 16) != (uint64_t)b->fsize) stream_offset(b, v, &k);
    b->ahead_block = (i64)k;
    return true;
}

// One record of the scan, as the selection loop of read_ranges sees it, from either source: the bytes in the host window (p), or a
// row of the device's record table (p == NULL; span is the row's, src the record's offset in the device window)
struct Rec { i64 bs; uint32_t rkey; i64 pos, l_name, n_cig, l_seq, span, src; const uint8_t* p; };

// the record at b->cur out of the host window.  *end: the stream ends at b->cur.  The checks and their order are the scan's own:
// the file ends inside the record's block_size, block_size < 32, the file ends inside the record
int next_host(csv_bam* b, Rec* r, bool* end)
{
    int rc;
    *end = false;
    const uint8_t* p = at(b, b->cur, 4, &rc);
    if (rc) return rc;
    if (!p) {
        if (b->cur != b->utotal) return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)b->cur);
        *end = true;
        return CSV_OK;
    }
    const i64 bs = rd_i32(p);
    if (bs < 32) return fail(b, CSV_E_INVALID, "%srecord with block_size < 32 at inflated byte %lld", "", (long long)b->cur);
    p = at(b, b->cur + 4, bs, &rc);
    if (rc) return rc;
    if (!p) return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)b->cur);
    r->bs = bs; r->rkey = (uint32_t)rd_i32(p); r->pos = rd_i32(p + 4); r->l_name = p[8]; r->n_cig = rd_u16(p + 12); r->l_seq = rd_u32(p + 16);
    r->span = -1; r->src = 0; r->p = p;
    return CSV_OK;
}

// the same from the rows of the device window: the window is loaded and framed from b->cur when its rows do not hold that offset
int next_framed(csv_bam* b, Rec* r, bool* end)
{
    *end = false;
    for (int round = 0; round < 8; round++) {
        const i64 cur = b->cur;
        if (b->fr_valid && (b->win_n == 0 || cur < b->fr_from || cur > b->fr_tail || csv_frame_window_serial(b->frame) != b->fr_serial)) b->fr_valid = false;
        if (b->fr_valid && cur < b->fr_tail) {
            const i64 o = cur - b->win_u0;
            i64 k = b->fr_i;
            if (!(k < b->fr_n && b->fr_rows[k].off == o)) {
                const csv::FrRow* e = b->fr_rows + b->fr_n;
                k = std::lower_bound(b->fr_rows, e, o, [](const csv::FrRow& x, i64 v) { return x.off < v; }) - b->fr_rows;
            }
            if (k < b->fr_n && b->fr_rows[k].off == o) {
                const csv::FrRow& w = b->fr_rows[k];
                b->fr_i = k + 1;
                r->bs = w.block_size; r->rkey = (uint32_t)w.refid; r->pos = w.pos; r->l_name = w.l_name; r->n_cig = w.n_cigar; r->l_seq = w.l_seq;
                r->span = w.span; r->src = w.off; r->p = nullptr;
                return CSV_OK;
            }
            b->fr_valid = false;                             // (not a start of the chain framed last: framed again from here)
        }
        i64 need = 4;
        if (cur == b->utotal) { *end = true; return CSV_OK; }
        if (cur + 4 > b->utotal) return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)cur);
        if (b->fr_valid && b->fr_tail_has_bs) {              // cur == fr_tail: the chain stopped here, at a record it could not step over
            const i64 bs = b->fr_tail_bs;
            if (bs < 32) return fail(b, CSV_E_INVALID, "%srecord with block_size < 32 at inflated byte %lld", "", (long long)cur);
            if (cur + 4 + bs > b->utotal) return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)cur);
            need = 4 + bs;
        }
        if (csv_frame_window_serial(b->frame) != b->fr_serial) b->win_n = 0;       // (another reader of the context loaded its window since)
        bool have;
        int rc = ensure(b, cur, need, &have);
        if (rc) return rc;
        b->t_off.clear(); b->t_len.clear();
        for (size_t j = b->win_b0; j < b->win_b1; j++) { b->t_off.push_back(b->blocks[j].uoff - b->win_u0); b->t_len.push_back((int32_t)b->blocks[j].isize); }
        csv::FrStitch R;
        rc = csv_frame_run(b->frame, (int32_t)b->t_off.size(), b->t_off.data(), b->t_len.data(), b->n_ref, cur - b->win_u0, &b->fr_rows, &R);
        if (rc) return fail(b, rc, "the device framing failed: %s", csv_last_error(b->frame));
        b->fr_n = R.n_records; b->fr_i = 0; b->fr_from = cur; b->fr_tail = b->win_u0 + R.tail;
        b->fr_tail_bs = R.tail_bs; b->fr_tail_has_bs = R.tail_has_bs != 0; b->fr_valid = true;
    }
    return fail(b, CSV_E_INVALID, "%sthe device framing made no progress at inflated byte %lld", "", (long long)b->cur);
}

// csv_bam_read / csv_bam_read_ranges: the records of contig `refid` that overlap one of the sorted, disjoint ranges, in file order
int read_ranges(csv_bam* b, int32_t refid, size_t nr, const int64_t* rbeg, const int64_t* rend, int64_t max_records, int32_t flags, csv_bam_chunk* out)
{
    const double t0 = now_ms();
    memset(out, 0, sizeof *out);
    b->ms_inflate = 0; b->inflated = b->compressed = 0;
    b->device_blocks = b->fallback_blocks = 0; b->ms_kernels = 0;
    b->slim.clear(); b->host.clear(); b->rec_off.clear(); b->host_off.clear(); b->rec_len.clear();
    b->pending.clear(); b->l_name_v.clear(); b->l_seq_v.clear(); b->slim_size = b->host_size = 0; b->framed_chunk = false;
    const bool framed = b->frame != nullptr;
    if (framed) { csv_frame_chunk_begin(b->frame, b); csv_frame_counters(b->frame, nullptr, nullptr, nullptr, nullptr, nullptr, 1); }
    const bool count_only = (flags & CSV_BAM_COUNT_ONLY) != 0;
    const uint32_t key = (uint32_t)refid;
    const bool indexed = b->has_index && refid >= 0 && refid < b->n_ref;
    const i64 beg = rbeg[0];
    size_t ri = b->range_i < nr ? b->range_i : nr - 1;
    bool done = false;                                       // the index says that nothing is left to read
    if (flags & CSV_BAM_RESTART) {                           // start of the contig if it was seen, else the last contig start before it
        ri = 0;
        b->seeked = false;
        b->ahead_block = -1;
        const i64 hint = b->hint_at >= 0 && b->hint_key == key && beg >= b->hint_beg ? b->hint_at : -1;
        if (indexed) {                                       // the linear-index entry of the first window, or the hint when that lies further on
            if (!index_seek(b, key, rbeg[0], rend[0], hint >= 0 ? hint : 0)) done = true;
        } else {
            b->cur = b->first_rec;
            auto it = b->contig_at.upper_bound(key);
            if (it != b->contig_at.begin()) { --it; b->cur = it->second; }
            if (hint >= 0) b->cur = hint;
        }
        b->hint_at = -1;
    }
    const bool set_hint = (flags & CSV_BAM_RESTART) != 0;
    i64 n = 0;
    bool more = false;
    int rc = CSV_OK;
    while (!done) {
        Rec r;
        bool at_end;
        rc = framed ? next_framed(b, &r, &at_end) : next_host(b, &r, &at_end);
        if (rc) return rc;
        if (at_end) {
            b->scanned_key = 0xffffffffu; b->scanned_any = true;
            break;
        }
        const uint8_t* p = r.p;
        const i64 bs = r.bs;
        const uint32_t rkey = r.rkey;
        if (!(b->seeked && rkey == b->seek_key)) {           // (a scan the index positioned does not see the first record of its contig)
            if (!b->contig_at.count(rkey)) b->contig_at[rkey] = b->cur;
            if (!b->scanned_any || rkey > b->scanned_key) { b->scanned_key = rkey; b->scanned_any = true; }
        }
        if (rkey > key) break;                               // the next contig (the unmapped tail sorts last): not consumed
        if (rkey < key) { b->cur += 4 + bs; continue; }
        const i64 pos = r.pos, l_name = r.l_name, n_cig = r.n_cig, l_seq = r.l_seq;
        const i64 fixed_to_aux = 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq;
        if (fixed_to_aux > bs) return fail(b, CSV_E_INVALID, "%srecord fields exceed its block_size at inflated byte %lld", "", (long long)b->cur);
        if (pos >= rend[ri]) {                               // sorted: nothing later can start before this range's end - on to the next range
            while (ri < nr && pos >= rend[ri]) ri++;
            if (ri == nr) { ri = nr - 1; break; }
            if (indexed) {
                if (!index_seek(b, key, rbeg[ri], rend[ri], b->cur)) break;
                continue;                                    // (the cursor may have moved: the record is read again)
            }
        }
        if (pos < rbeg[ri]) {                                // overlaps the range only if it reaches past its begin (and then no later one: they are disjoint)
            const i64 beg = rbeg[ri];
            i64 span = r.span;                               // (the row's on the framing route)
            if (p) {
                span = 0;
                const uint8_t* cg = p + 32 + l_name;
                for (i64 k = 0; k < n_cig; k++) {
                    const uint32_t w = rd_u32(cg + 4 * k);
                    const uint32_t op = w & 15u;
                    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += w >> 4;
                }
            }
            if (pos + (span ? span : 1) <= beg) { b->cur += 4 + bs; continue; }
        }
        if (n == max_records) { more = true; break; }
        // (every record in front of this one ends at or before the begin of the range it is emitted for: those tested against an
        // earlier range end before that range's begin, those the index jumped over overlap no window from this range's on)
        if (n == 0 && set_hint) { b->hint_key = key; b->hint_beg = rbeg[ri]; b->hint_at = b->cur; }
        if (!count_only && framed) {                         // the same layout, in the device images: packed when the window is left
            const i64 aux_len = bs - fixed_to_aux, slim_len = 32 + 4 * n_cig + aux_len;
            csv::FrPack q{};
            q.src = r.src; q.rec_off = b->slim_size; q.host_off = b->host_size; q.bs = (int32_t)bs; q.l_seq = (uint32_t)l_seq; q.n_cig = (uint16_t)n_cig; q.l_name = (uint8_t)l_name;
            b->pending.push_back(q);
            b->rec_off.push_back(b->slim_size); b->rec_len.push_back((uint32_t)slim_len); b->host_off.push_back(b->host_size);
            b->l_name_v.push_back((int32_t)l_name); b->l_seq_v.push_back((int32_t)(uint32_t)l_seq);
            b->slim_size += (slim_len + SLIM_ALIGN - 1) / SLIM_ALIGN * SLIM_ALIGN;
            b->host_size += l_name + (l_seq + 1) / 2;
        } else if (!count_only) {
            const i64 aux_len = bs - fixed_to_aux, slim_len = 32 + 4 * n_cig + aux_len;
            const size_t s0 = b->slim.size();
            b->rec_off.push_back((i64)s0);
            b->rec_len.push_back((uint32_t)slim_len);
            b->slim.resize(s0 + (size_t)((slim_len + SLIM_ALIGN - 1) / SLIM_ALIGN * SLIM_ALIGN));
            uint8_t* d = b->slim.data() + s0;
            memcpy(d, p, 32);
            memcpy(d + 32, p + 32 + l_name, (size_t)(4 * n_cig));
            memcpy(d + 32 + 4 * n_cig, p + fixed_to_aux, (size_t)aux_len);
            memset(d + slim_len, 0, b->slim.size() - s0 - (size_t)slim_len);
            const size_t h0 = b->host.size();
            b->host_off.push_back((i64)h0);
            b->host.resize(h0 + (size_t)(l_name + (l_seq + 1) / 2));
            memcpy(b->host.data() + h0, p + 32, (size_t)l_name);
            memcpy(b->host.data() + h0 + l_name, p + 32 + l_name + 4 * n_cig, (size_t)((l_seq + 1) / 2));
        }
        n++;
        out->record_bytes += 4 + bs;
        b->cur += 4 + bs;
    }
    b->range_i = ri;
    if (framed) {
        rc = frame_flush(b);
        if (rc) return rc;
        if (!count_only) {
            rc = csv_frame_chunk_end(b->frame, n, b->rec_off.data(), b->rec_len.data(), b->host_off.data(), b->l_name_v.data(), b->l_seq_v.data());
            if (rc) return fail(b, rc, "the device framing failed: %s", csv_last_error(b->frame));
            b->framed_chunk = true;
        }
    }
    b->host_off.push_back(framed ? b->host_size : (i64)b->host.size());
    out->n_records = n; out->more = more ? 1 : 0;
    out->slim = framed ? nullptr : b->slim.data(); out->slim_bytes = framed ? b->slim_size : (int64_t)b->slim.size();
    out->rec_off = b->rec_off.data(); out->rec_len = b->rec_len.data();
    out->host = framed ? nullptr : b->host.data(); out->host_bytes = framed ? b->host_size : (int64_t)b->host.size(); out->host_off = b->host_off.data();
    out->inflated_bytes = b->inflated; out->compressed_bytes = b->compressed;
    out->ms_inflate = b->ms_inflate; out->ms_frame = now_ms() - t0 - b->ms_inflate;
    return CSV_OK;
}

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


// ---- the index build (index_core.h)
struct IxTables { std::vector<csv::ix_i64> uoff, coff, l_ref; std::vector<uint32_t> isize; };

int index_refuse(csv_bam* b, long long ordinal, int why)
{
    char buf[256];
    snprintf(buf, sizeof buf, "cannot build the index: record %lld %s", ordinal, csv::ix_refusal_text(why));
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
        const i64 cg = 32 + r.l_name;                        // the span of the record's own CIGAR words, read inside the record only (fr_row's rule)
        i64 n_in = cg <= r.bs ? (r.bs - cg) / 4 : 0, span = 0;
        if (n_in > r.n_cig) n_in = r.n_cig;
        for (i64 k = 0; k < n_in; k++) {
            const uint32_t w = rd_u32(r.p + cg + 4 * k), op = w & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += w >> 4;
        }
        const csv::IxRec x = csv::ix_record(r.pos, span);
        const int why = csv::ix_refuse((int32_t)r.rkey, r.pos, x, b->n_ref, T.l_ref.data(), B->prev);
        if (why) return index_refuse(b, B->records, why);
        B->add_record((int32_t)r.rkey, r.pos, x, (rd_u16(r.p + 14) & 4) != 0, csv::ix_voff(blocks, b->cur), csv::ix_voff(blocks, b->cur + 4 + r.bs));
        b->cur += 4 + r.bs;
    }
}

// the framing route: window by window, the rows stay on the device (csv_frame_run without a row pointer) and the index kernels read
// them there; the verdict and the runs come down.  The checks of the chain and their texts are next_framed's.
int index_build_device(csv_bam* b, const IxTables& T, csv::ix::Builder* B)
{
    int rc = csv_index_begin(b->frame, b->n_ref, T.l_ref.data(), (int64_t)T.uoff.size(), T.uoff.data(), T.coff.data(), T.isize.data());
    if (rc) return fail(b, rc, "the device index build failed: %s", csv_last_error(b->frame));
    csv::IxCarry carry{0, 0, 0, 0};
    bool tail_has_bs = false;
    i64 tail_bs = 0;
    int idle = 0;
    b->fr_valid = false;
    for (;;) {
        const i64 cur = b->cur;
        if (cur == b->utotal) break;
        if (cur + 4 > b->utotal) return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)cur);
        i64 need = 4;
        if (tail_has_bs) {                                   // the chain stopped here, at a record it could not step over
            if (tail_bs < 32) return fail(b, CSV_E_INVALID, "%srecord with block_size < 32 at inflated byte %lld", "", (long long)cur);
            if (cur + 4 + tail_bs > b->utotal) return fail(b, CSV_E_INVALID, "%sthe file ends inside a record (at inflated byte %lld)", "", (long long)cur);
            need = 4 + tail_bs;
        }
        if (csv_frame_window_serial(b->frame) != b->fr_serial) b->win_n = 0;
        bool have;
        rc = ensure(b, cur, need, &have);
        if (rc) return rc;
        b->t_off.clear(); b->t_len.clear();
        for (size_t j = b->win_b0; j < b->win_b1; j++) { b->t_off.push_back(b->blocks[j].uoff - b->win_u0); b->t_len.push_back((int32_t)b->blocks[j].isize); }
        csv::FrStitch R;
        rc = csv_frame_run(b->frame, (int32_t)b->t_off.size(), b->t_off.data(), b->t_len.data(), b->n_ref, cur - b->win_u0, nullptr, &R);
        if (rc) return fail(b, rc, "the device framing failed: %s", csv_last_error(b->frame));
        b->ix_frame_runs++;
        if (R.n_records > 0) {
            csv::IxVerdict V;
            const csv::IxRun* runs = nullptr;
            rc = csv_index_window(b->frame, R.n_records, b->win_u0, B->records, &carry, &V, &runs);
            if (rc) return fail(b, rc, "the device index build failed: %s", csv_last_error(b->frame));
            if (V.bad != csv::IX_NONE) return index_refuse(b, (long long)(V.bad >> 3), (int)(V.bad & 7));
            for (i64 k = 0; k < V.n_runs; k++) B->add_run(runs[k]);
            b->ix_runs += V.n_runs;
            B->records += R.n_records;
            carry = V.last;
        }
        const i64 tail = b->win_u0 + R.tail;
        if (tail > cur) idle = 0;
        else if (++idle > 4) return fail(b, CSV_E_INVALID, "%sthe device framing made no progress at inflated byte %lld", "", (long long)cur);
        tail_has_bs = R.tail_has_bs != 0; tail_bs = R.tail_bs;
        b->cur = tail;
    }
    rc = csv_index_end(b->frame, B->lin.data(), (int64_t)B->lin.size(), B->counts.data(), (int64_t)B->counts.size());
    if (rc) return fail(b, rc, "the device index build failed: %s", csv_last_error(b->frame));
    return CSV_OK;
}

}  // namespace

extern "C" {

int csv_bam_index_build(csv_bam* b, int32_t flags, int64_t* n_bytes)
{
    if (!b || flags != 0) return CSV_E_INVALID;
    if (n_bytes) *n_bytes = 0;
    // the build is a read: the chunk handed out last is dead, the counters start over, the scan state of a region is forgotten
    b->ms_inflate = 0; b->inflated = b->compressed = 0;
    b->device_blocks = b->fallback_blocks = 0; b->ms_kernels = 0;
    b->slim.clear(); b->host.clear(); b->rec_off.clear(); b->host_off.clear(); b->rec_len.clear();
    b->pending.clear(); b->l_name_v.clear(); b->l_seq_v.clear(); b->slim_size = b->host_size = 0; b->framed_chunk = false;
    if (b->frame) { csv_frame_chunk_begin(b->frame, b); csv_frame_counters(b->frame, nullptr, nullptr, nullptr, nullptr, nullptr, 1); }
    b->seeked = false; b->ahead_block = -1; b->hint_at = -1; b->range_i = 0;
    b->ix_records = b->ix_runs = b->ix_frame_runs = b->ix_windows = b->ix_up = b->ix_down = 0; b->ix_ms_kernels = 0;
    IxTables T;
    for (const Block& k : b->blocks) { T.uoff.push_back(k.uoff); T.coff.push_back(k.coff); T.isize.push_back(k.isize); }
    T.l_ref.assign(b->lengths.begin(), b->lengths.end());
    csv::ix::Builder B;
    B.begin(b->n_ref, T.l_ref.data());
    b->cur = b->first_rec;
    const int rc = b->frame ? index_build_device(b, T, &B) : index_build_host(b, T, &B);
    b->ix_ms_kernels = b->ms_kernels;
    if (b->frame) {
        double ms_f = 0, ms_x = 0;
        int64_t dn_f = 0, up_f = 0, dn_x = 0, up_x = 0, wins = 0;
        csv_frame_counters(b->frame, nullptr, nullptr, &ms_f, &dn_f, &up_f, 0);
        csv_index_counters(b->frame, &ms_x, &dn_x, &up_x, &wins);
        b->ix_ms_kernels += ms_f + ms_x; b->ix_down = dn_f + dn_x; b->ix_up = up_f + up_x; b->ix_windows = wins;
    }
    b->cur = b->first_rec;
    b->win_n = 0; b->fr_valid = false;                       // (what a later read costs does not depend on what the build left in the window)
    if (rc) return rc;
    b->ix_records = B.records;
    if (!b->frame) b->ix_runs = (i64)B.runs.size();
    // the built bytes take the path a file's bytes take: parsed and validated against this file's blocks, then installed
    std::vector<uint8_t> bytes = B.bytes();
    bai::Index ix;
    std::string err;
    if (!bai::parse(bytes.data(), bytes.size(), b->n_ref, "the built index", voff_check, b, &ix, &err)) {
        b->err = "cannot build the index: " + err;
        return CSV_E_INVALID;
    }
    b->index = std::move(ix);
    b->has_index = true;
    b->index_built = true; b->index_bytes = std::move(bytes);
    b->hint_at = -1; b->ahead_block = -1;
    if (n_bytes) *n_bytes = (int64_t)b->index_bytes.size();
    return CSV_OK;
}

int csv_bam_index_bytes(const csv_bam* b, uint8_t* out, int64_t cap, int64_t* need)
{
    if (!b) return CSV_E_INVALID;
    if (need) *need = 0;
    if (!b->has_index || !b->index_built) return CSV_E_STATE;
    if (need) *need = (int64_t)b->index_bytes.size();
    if (!out || cap < (int64_t)b->index_bytes.size()) return CSV_E_CAPACITY;
    memcpy(out, b->index_bytes.data(), b->index_bytes.size());
    return CSV_OK;
}

int csv_bam_index_build_stats(const csv_bam* b, int64_t* records, int64_t* runs, double* ms_kernels, int64_t* bytes_up, int64_t* bytes_down, int64_t* frame_runs,
                              int64_t* index_windows)
{
    if (!b) return CSV_E_INVALID;
    if (records) *records = b->ix_records;
    if (runs) *runs = b->ix_runs;
    if (ms_kernels) *ms_kernels = b->ix_ms_kernels;
    if (bytes_up) *bytes_up = b->ix_up;
    if (bytes_down) *bytes_down = b->ix_down;
    if (frame_runs) *frame_runs = b->ix_frame_runs;
    if (index_windows) *index_windows = b->ix_windows;
    return CSV_OK;
}

}  // extern "C"

extern "C" {

int csv_bam_read(csv_bam* b, int32_t refid, int64_t beg, int64_t end, int64_t max_records, int32_t flags, csv_bam_chunk* out)
{
    if (!b || !out || max_records < 1) return CSV_E_INVALID;
    b->range_i = 0;
    return read_ranges(b, refid, 1, &beg, &end, max_records, flags, out);
}

int csv_bam_read_ranges(csv_bam* b, int32_t refid, int32_t n_ranges, const int64_t* beg, const int64_t* end, int64_t max_records, int32_t flags, csv_bam_chunk* out)
{
    if (!b || !out || max_records < 1 || n_ranges < 1 || !beg || !end) return CSV_E_INVALID;
    for (int32_t i = 0; i < n_ranges; i++)
        if (beg[i] > end[i] || (i && beg[i] < end[i - 1])) return fail(b, CSV_E_INVALID, "%sthe ranges of a read must be sorted and disjoint (range %lld)", "", i);
    return read_ranges(b, refid, (size_t)n_ranges, beg, end, max_records, flags, out);
}

int csv_bam_index_load(csv_bam* b, const char* path)
{
    if (!b) return CSV_E_INVALID;
    std::vector<std::string> tries;
    if (path) tries.push_back(path);
    else {
        tries.push_back(b->path + ".bai");
        if (b->path.size() > 4 && b->path.compare(b->path.size() - 4, 4, ".bam") == 0) tries.push_back(b->path.substr(0, b->path.size() - 4) + ".bai");
    }
    for (const std::string& t : tries) {
        std::vector<uint8_t> data;
        if (!read_file(t, &data)) continue;
        bai::Index ix;
        std::string err;
        if (!bai::parse(data.data(), data.size(), b->n_ref, t.c_str(), voff_check, b, &ix, &err)) {
            csv_bam_index_drop(b);                           // a reader whose load failed has no index, whatever it had
            b->err = err;
            return CSV_E_INVALID;
        }
        b->index = std::move(ix);
        b->has_index = true;
        b->index_built = false; b->index_bytes.clear();
        b->hint_at = -1; b->ahead_block = -1;
        return CSV_OK;
    }
    b->err = path ? std::string("cannot read the index ") + path : "no index beside " + b->path + " (" + tries[0] + (tries.size() > 1 ? ", " + tries[1] : "") + ")";
    return CSV_E_STATE;
}

int64_t csv_bam_index_block(const csv_bam* b, int32_t refid, int64_t beg)
{
    if (!b || !b->has_index || refid < 0 || refid >= b->n_ref) return -2;
    uint64_t v;
    if (!bai::start_offset(b->index, refid, beg, &v)) return -1;
    if ((v >> 16) == (uint64_t)b->fsize) return (int64_t)b->blocks.size() - 1;
    size_t k;
    stream_offset(b, v, &k);
    return (int64_t)k;
}

int csv_bam_index_drop(csv_bam* b)
{
    if (!b) return CSV_E_INVALID;
    b->index = bai::Index();
    b->has_index = false;
    b->index_built = false; b->index_bytes.clear();
    b->hint_at = -1; b->ahead_block = -1; b->seeked = false;
    return CSV_OK;
}

int csv_bam_index_stats(const csv_bam* b, int64_t* mapped, int64_t* unmapped, int64_t* n_no_coor)
{
    if (!b) return CSV_E_INVALID;
    if (!b->has_index) return CSV_E_STATE;
    for (int32_t r = 0; r < b->n_ref; r++) {
        if (mapped) mapped[r] = (int64_t)b->index.refs[(size_t)r].n_mapped;
        if (unmapped) unmapped[r] = (int64_t)b->index.refs[(size_t)r].n_unmapped;
    }
    if (n_no_coor) *n_no_coor = b->index.has_no_coor ? (int64_t)b->index.n_no_coor : -1;
    return CSV_OK;
}

}  // extern "C"
