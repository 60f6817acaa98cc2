// stage_ref.hip.h — csv_ref_gather: base ranges of the contigs of a BGZF-compressed FASTA out of the blocks they touch (DESIGN.md
// section 35).  The blocks are inflated through inflate_impl with dev_out, so their bytes stay in device memory; k_ref_gather (at the
// end of bam.hip.h, over ref_core.h) cuts the ranges out of them, one wavefront per output tile; only the bases come back.
// csv_ref_gather_host is the same over blocks the caller has inflated already: ref_core.h's host form on one thread.  The device
// buffers are RefState's own (ctx.hip.h) and the inflate's: no arena is planned, no generation word moves, and nothing another stage
// left on the device is touched.  Behind them csv_fai_events / csv_fai_events_host: a window of the text as the event rows its .fai is
// assembled from (k_fai_tiles, k_fai_events).  Host code; included by cutesv_hip.hip behind stage_deflate.hip.h.

namespace {

// What both entries check before anything runs - the kernel and the host form trust it - and the tables both need: out_off (where a
// range's bases start, n_ranges + 1) and tile_first (the tiles in front of a range, n_ranges + 1).  -> "" or the refusal's text.
std::string ref_check(const char* who, int32_t n_blocks, const int64_t* uoff, const int32_t* isize, int64_t n_ranges, const int64_t* base_off, const int32_t* line_bases,
                      const int32_t* line_width, const int64_t* beg, const int64_t* end, const int64_t* data_off, std::vector<ref_i64>& out_off, std::vector<ref_i64>& tile_first)
{
    char buf[256];
    auto say = [&](const char* fmt, long long a, long long b) { snprintf(buf, sizeof buf, fmt, who, a, b); return std::string(buf); };
    constexpr int64_t FAR = (int64_t)1 << 60;                     // offsets beyond this are no file's: the sums below cannot overflow
    for (int32_t k = 0; k < n_blocks; k++) {
        if (isize[k] < 0 || isize[k] > 65536) return say("%s: isize of block %lld is %lld (0 .. 65536)", k, isize[k]);
        if (uoff[k] < 0 || uoff[k] > FAR) return say("%s: uoff of block %lld is %lld", k, uoff[k]);
        if (k > 0 && uoff[k - 1] + isize[k - 1] > uoff[k]) return say("%s: blocks %lld and %lld overlap or are not sorted by uoff", k - 1, k);
    }
    out_off.assign((size_t)n_ranges + 1, 0);
    tile_first.assign((size_t)n_ranges + 1, 0);
    // block k's bytes start at data_off[k]: the sizes' running sum on the device route, the caller's table on the host route; the
    // coverage test reads no byte, so it needs none of that
    const RefBlocks B{(int)n_blocks, (const ref_i64*)uoff, isize, (const ref_i64*)data_off, nullptr};
    for (int64_t r = 0; r < n_ranges; r++) {
        if (line_bases[r] <= 0) return say("%s: line_bases of range %lld is %lld", r, line_bases[r]);
        if (line_width[r] < line_bases[r]) return say("%s: line_width of range %lld is below its line_bases (%lld)", r, line_bases[r]);
        if (beg[r] < 0 || end[r] < beg[r]) return say("%s: range %lld has beg %lld below 0 or beyond its end", r, beg[r]);
        if (base_off[r] < 0 || base_off[r] > FAR) return say("%s: base_off of range %lld is %lld", r, base_off[r]);
        if ((__int128)base_off[r] + (__int128)(end[r] / line_bases[r] + 1) * line_width[r] > (__int128)FAR) return say("%s: range %lld ends at base %lld, beyond any file", r, end[r]);
        if (!ref_covered(B, base_off[r], line_bases[r], line_width[r], beg[r], end[r])) return say("%s: range %lld reads bytes that lie in none of the %lld blocks", r, n_blocks);
        out_off[(size_t)r + 1] = out_off[(size_t)r] + (end[r] - beg[r]);
        tile_first[(size_t)r + 1] = tile_first[(size_t)r] + ref_tiles(end[r] - beg[r]);
        if (out_off[(size_t)r + 1] > FAR) return say("%s: the ranges up to %lld hold %lld bases", r, out_off[(size_t)r + 1]);
    }
    return std::string();
}

bool ref_null_args(int32_t n_blocks, int64_t n_ranges, const void* uoff, const void* isize, const void* base_off, const void* lb, const void* lw, const void* beg, const void* end,
                   const void* out_off, const void* out_bytes)
{
    return !out_bytes || !out_off || (n_blocks > 0 && (!uoff || !isize)) || (n_ranges > 0 && (!base_off || !lb || !lw || !beg || !end));
}

}  // namespace

extern "C" {

int csv_ref_gather(csv_ctx* c, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, const int64_t* uoff, const int32_t* isize,
                   const uint32_t* crc, int64_t n_ranges, const int64_t* base_off, const int32_t* line_bases, const int32_t* line_width, const int64_t* beg, const int64_t* end,
                   uint8_t* out, int64_t out_cap, int64_t* out_off, int64_t* out_bytes, uint8_t* block_status, int32_t flags, double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (n_blocks < 0 || n_ranges < 0 || comp_bytes < 0 || out_cap < 0) return fail(c, CSV_E_INVALID, "csv_ref_gather: a negative count");
    if (flags != 0) return fail(c, CSV_E_INVALID, "csv_ref_gather: flags must be 0");
    if (ref_null_args(n_blocks, n_ranges, uoff, isize, base_off, line_bases, line_width, beg, end, out_off, out_bytes) ||
        (n_blocks > 0 && (!in_off || !in_len || !crc || !block_status)) || (comp_bytes > 0 && !comp) || (out_cap > 0 && !out))
        return fail(c, CSV_E_INVALID, "csv_ref_gather: a null pointer");
    RefState& s = c->ref;
    const std::string why = ref_check("csv_ref_gather", n_blocks, uoff, isize, n_ranges, base_off, line_bases, line_width, beg, end, nullptr, s.out_off, s.tile_first);
    if (!why.empty()) return fail(c, CSV_E_INVALID, "%s", why.c_str());
    for (int32_t k = 0; k < n_blocks; k++)
        if (in_len[k] < 0 || in_off[k] < 0 || in_off[k] > comp_bytes - in_len[k]) return fail(c, CSV_E_INVALID, "csv_ref_gather: the payload of block %d lies outside comp", (int)k);
    const size_t nr = (size_t)n_ranges, nb = (size_t)n_blocks;
    const int64_t total = s.out_off[nr], n_tiles = s.tile_first[nr];
    if (ms_kernels) ms_kernels[0] = ms_kernels[1] = 0;
    memcpy(out_off, s.out_off.data(), 8 * (nr + 1));
    *out_bytes = total;
    if (total > out_cap) return CSV_OK;                            // the caller learns the need; `out` and block_status stay as they are
    if (n_blocks > 0) memset(block_status, 0, nb);
    if (total == 0) return CSV_OK;                                 // nothing to read: nothing is inflated
    // the blocks inflate back to back into s.data
    s.data_off.assign(nb + 1, 0);
    for (size_t k = 0; k < nb; k++) s.data_off[k + 1] = s.data_off[k] + isize[k];
    const int64_t data_bytes = s.data_off[nb];
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TRY(reserve(c, s.data, (size_t)data_bytes + 8));
    double ms_inf = 0;
    TRY(inflate_impl(c, comp, comp_bytes, n_blocks, in_off, in_len, s.data_off.data(), isize, crc, nullptr, dp<uint8_t>(s.data), data_bytes, 0, block_status, &ms_inf));
    // tab: per block uoff, data_off (8 bytes each), isize (4); per range out_off, tile_first (8 each, n + 1), base_off, beg (8), lb, lw (4)
    const size_t o_doff = 8 * nb, o_isize = 16 * nb, o_out = (20 * nb + 7) / 8 * 8, o_tile = o_out + 8 * (nr + 1), o_base = o_tile + 8 * (nr + 1), o_beg = o_base + 8 * nr,
                 o_lb = o_beg + 8 * nr, o_lw = o_lb + 4 * nr, tab_bytes = o_lw + 4 * nr;
    s.tab_h.resize(tab_bytes);
    char* h = s.tab_h.data();
    memcpy(h, uoff, 8 * nb); memcpy(h + o_doff, s.data_off.data(), 8 * nb); memcpy(h + o_isize, isize, 4 * nb);
    memcpy(h + o_out, s.out_off.data(), 8 * (nr + 1)); memcpy(h + o_tile, s.tile_first.data(), 8 * (nr + 1));
    memcpy(h + o_base, base_off, 8 * nr); memcpy(h + o_beg, beg, 8 * nr); memcpy(h + o_lb, line_bases, 4 * nr); memcpy(h + o_lw, line_width, 4 * nr);
    TRY(reserve(c, s.tab, tab_bytes));
    TRY(reserve(c, s.out, (size_t)total + 8));
    TRY(h2d(c, s.tab, h, (i64)tab_bytes));
    char* t = (char*)s.tab.p;
    const RefGatherArgs A{RefBlocks{(int)n_blocks, (const ref_i64*)t, (const int*)(t + o_isize), (const ref_i64*)(t + o_doff), dp<uint8_t>(s.data)}, (i64)n_ranges, (i64)n_tiles,
                          (const i64*)(t + o_tile), (const i64*)(t + o_out), (const i64*)(t + o_base), (const int*)(t + o_lb), (const int*)(t + o_lw), (const i64*)(t + o_beg),
                          dp<uint8_t>(s.out)};
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(k_ref_gather, dim3((unsigned)std::min<int64_t>((n_tiles + 3) / 4, 8192)), dim3(256), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[3], st));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, s.out.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (ms_kernels) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        ms_kernels[0] = ms_inf; ms_kernels[1] = ms;
    }
    return CSV_OK;
}

int csv_ref_gather_host(const uint8_t* data, int64_t data_bytes, int32_t n_blocks, const int64_t* data_off, const int64_t* uoff, const int32_t* isize, int64_t n_ranges,
                        const int64_t* base_off, const int32_t* line_bases, const int32_t* line_width, const int64_t* beg, const int64_t* end, uint8_t* out, int64_t out_cap,
                        int64_t* out_off, int64_t* out_bytes, char* err, int32_t err_cap)
{
    auto refuse = [&](const std::string& why) { if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", why.c_str()); return CSV_E_INVALID; };
    if (err && err_cap > 0) err[0] = 0;
    if (n_blocks < 0 || n_ranges < 0 || data_bytes < 0 || out_cap < 0) return refuse("csv_ref_gather_host: a negative count");
    if (ref_null_args(n_blocks, n_ranges, uoff, isize, base_off, line_bases, line_width, beg, end, out_off, out_bytes) || (n_blocks > 0 && !data_off) || (data_bytes > 0 && !data) ||
        (out_cap > 0 && !out))
        return refuse("csv_ref_gather_host: a null pointer");
    std::vector<ref_i64> oo, tf;
    const std::string why = ref_check("csv_ref_gather_host", n_blocks, uoff, isize, n_ranges, base_off, line_bases, line_width, beg, end, data_off, oo, tf);
    if (!why.empty()) return refuse(why);
    for (int32_t k = 0; k < n_blocks; k++)
        if (data_off[k] < 0 || data_off[k] > data_bytes - isize[k]) return refuse("csv_ref_gather_host: the bytes of block " + std::to_string(k) + " lie outside data");
    memcpy(out_off, oo.data(), 8 * ((size_t)n_ranges + 1));
    *out_bytes = oo[(size_t)n_ranges];
    if (*out_bytes > out_cap) return CSV_OK;
    const RefBlocks B{(int)n_blocks, (const ref_i64*)uoff, isize, (const ref_i64*)data_off, data};
    const RefOneLane L;
    for (int64_t t = 0; t < tf[(size_t)n_ranges]; t++)
        ref_gather_tile(L, B, (ref_i64)n_ranges, tf.data(), oo.data(), (const ref_i64*)base_off, line_bases, line_width, (const ref_i64*)beg, (ref_i64)t, out);
    return CSV_OK;
}

}  // extern "C"

// ---- the event rows of a window of FASTA text (the .fai of a BGZF-compressed FASTA on the device route)
namespace {

// the header texts of a window [base, base + n): per header row, then for a header in progress behind the window, the bytes of that
// line inside the window -> visit(window-relative first byte, bytes); the sum of the bytes is returned
template <class F> int64_t fai_header_pieces(const FaiRow* rows, int64_t n_rows, const FaiCarry& tail, int64_t base, int64_t n, F visit)
{
    int64_t sum = 0;
    auto piece = [&](int64_t s, int64_t e) { const int64_t s0 = s < base ? base : s; if (e > s0) { visit(s0 - base, e - s0); sum += e - s0; } };
    for (int64_t i = 0; i < n_rows; i++)
        if (rows[i].bases & FAI_HDR) piece(rows[i].start, rows[i].start + rows[i].bytes);
    if (tail.first == '>' && tail.start < base + n) piece(tail.start, base + n);
    return sum;
}

bool fai_bad_args(int64_t base, const int64_t* carry, const int64_t* rows, int64_t row_cap, const int64_t* n_rows, const int64_t* tail, const char* hdr, int64_t hdr_cap,
                  const int64_t* hdr_bytes)
{
    return base < 0 || row_cap < 0 || hdr_cap < 0 || !carry || !n_rows || !tail || !hdr_bytes || (row_cap > 0 && !rows) || (hdr_cap > 0 && !hdr) || carry[0] < 0 || carry[0] > base;
}

}  // namespace

extern "C" {

// The blocks of a window, whose text starts at absolute offset `base`, are inflated on the device and stay there; k_fai_tiles and
// k_fai_events (bam.hip.h) turn the text into ref_core.h's event rows; the rows (3 int64 each), the carry behind the window (tail[3])
// and the header texts come back.  carry[3]: csv_fasta_index_stream_carry's.  *n_rows > row_cap or *hdr_bytes > hdr_cap: the need is
// reported and neither `rows` nor `hdr` is written; *n_rows = -1: a block has a non-zero status.  In both cases the window is the
// host form's to index (csv_fasta_index_stream_feed).  ms_kernels[2]: inflate, events.
int csv_fai_events(csv_ctx* c, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, const int32_t* isize, const uint32_t* crc,
                   int64_t base, const int64_t* carry, int64_t* rows, int64_t row_cap, int64_t* n_rows, int64_t* tail, char* hdr, int64_t hdr_cap, int64_t* hdr_bytes,
                   uint8_t* block_status, double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (n_blocks < 0 || comp_bytes < 0) return fail(c, CSV_E_INVALID, "csv_fai_events: a negative count");
    if (fai_bad_args(base, carry, rows, row_cap, n_rows, tail, hdr, hdr_cap, hdr_bytes) || (n_blocks > 0 && (!in_off || !in_len || !isize || !crc || !block_status)) ||
        (comp_bytes > 0 && !comp))
        return fail(c, CSV_E_INVALID, "csv_fai_events: a null pointer, or a carry that starts behind the window");
    RefState& s = c->ref;
    const size_t nb = (size_t)n_blocks;
    s.data_off.assign(nb + 1, 0);
    for (size_t k = 0; k < nb; k++) {
        if (isize[k] < 0 || isize[k] > 65536) return fail(c, CSV_E_INVALID, "csv_fai_events: isize of block %d is %d (0 .. 65536)", (int)k, (int)isize[k]);
        if (in_len[k] < 0 || in_off[k] < 0 || in_off[k] > comp_bytes - in_len[k]) return fail(c, CSV_E_INVALID, "csv_fai_events: the payload of block %d lies outside comp", (int)k);
        s.data_off[k + 1] = s.data_off[k] + isize[k];
    }
    const int64_t n = s.data_off[nb];
    if (n > ((int64_t)1 << 30)) return fail(c, CSV_E_INVALID, "csv_fai_events: a window of %lld bytes (at most 2^30)", (long long)n);
    if (ms_kernels) ms_kernels[0] = ms_kernels[1] = 0;
    *n_rows = 0; *hdr_bytes = 0;
    memcpy(tail, carry, 24);
    if (n_blocks > 0) memset(block_status, 0, nb);
    if (n == 0) return CSV_OK;                                     // no text: the line in progress goes on
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TRY(reserve(c, s.data, (size_t)n + 8));
    double ms_inf = 0;
    TRY(inflate_impl(c, comp, comp_bytes, n_blocks, in_off, in_len, s.data_off.data(), isize, crc, nullptr, dp<uint8_t>(s.data), n, 0, block_status, &ms_inf));
    if (ms_kernels) ms_kernels[0] = ms_inf;
    for (size_t k = 0; k < nb; k++)
        if (block_status[k]) { *n_rows = -1; return CSV_OK; }
    const int n_tiles = (int)((n + FAI_TILE - 1) / FAI_TILE);
    const size_t o_cnt = 16 * (size_t)n_tiles, o_out = o_cnt + 16 * (size_t)n_tiles;
    TRY(reserve(c, s.fai, o_out + sizeof(FaiOut)));
    TRY(reserve(c, s.fai_rows, (size_t)row_cap * sizeof(FaiRow) + 8));
    char* t = (char*)s.fai.p;
    const FaiArgs A{dp<uint8_t>(s.data), (i64)n, (i64)base, FaiCarry{carry[0], carry[1], carry[2]}, n_tiles, (i64*)t, (int*)(t + o_cnt), dp<FaiRow>(s.fai_rows), (i64)row_cap,
                    (FaiOut*)(t + o_out)};
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(k_fai_tiles, dim3((unsigned)n_tiles), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_fai_events<false>, dim3((unsigned)n_tiles), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_fai_events<true>, dim3((unsigned)n_tiles), dim3(256), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[3], st));
    HIP_TRY(c, hipGetLastError());
    FaiOut out;
    HIP_TRY(c, hipMemcpyAsync(&out, t + o_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (ms_kernels) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        ms_kernels[1] = ms;
    }
    *n_rows = out.n_rows;
    tail[0] = out.tail.start; tail[1] = out.tail.first; tail[2] = out.tail.last;
    if (out.n_rows < 0 || out.tail.start < carry[0] || out.tail.start > base + n) return fail(c, CSV_E_STATE, "csv_fai_events: the kernel's totals do not describe the window");
    if (out.n_rows > row_cap) return CSV_OK;
    if (out.n_rows > 0) {
        HIP_TRY(c, hipMemcpyAsync(rows, s.fai_rows.p, (size_t)out.n_rows * sizeof(FaiRow), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    const FaiRow* R = (const FaiRow*)rows;
    *hdr_bytes = fai_header_pieces(R, out.n_rows, out.tail, base, n, [](int64_t, int64_t) {});
    if (*hdr_bytes > hdr_cap) return CSV_OK;
    int64_t at = 0;
    hipError_t e = hipSuccess;
    fai_header_pieces(R, out.n_rows, out.tail, base, n, [&](int64_t s0, int64_t len) {
        // (a row the kernel wrote lies inside the window; a piece that does not is not copied)
        if (e == hipSuccess && s0 >= 0 && len <= n - s0 && len <= hdr_cap - at) e = hipMemcpyAsync(hdr + at, dp<uint8_t>(s.data) + s0, (size_t)len, hipMemcpyDeviceToHost, st);
        at += len;
    });
    if (e != hipSuccess) return fail(c, CSV_E_HIP, "the header texts' copy failed: %s", hipGetErrorString(e));
    HIP_TRY(c, hipStreamSynchronize(st));
    return CSV_OK;
}

// the same from a window the caller has inflated: ref_core.h's host form
int csv_fai_events_host(const uint8_t* data, int64_t n, int64_t base, const int64_t* carry, int64_t* rows, int64_t row_cap, int64_t* n_rows, int64_t* tail, char* hdr, int64_t hdr_cap,
                        int64_t* hdr_bytes)
{
    if (n < 0 || (n > 0 && !data) || fai_bad_args(base, carry, rows, row_cap, n_rows, tail, hdr, hdr_cap, hdr_bytes)) return CSV_E_INVALID;
    FaiCarry tl;
    *n_rows = fai_events_host(data, n, base, FaiCarry{carry[0], carry[1], carry[2]}, (FaiRow*)rows, row_cap, &tl);
    tail[0] = tl.start; tail[1] = tl.first; tail[2] = tl.last;
    *hdr_bytes = 0;
    if (*n_rows > row_cap) return CSV_OK;
    *hdr_bytes = fai_header_pieces((const FaiRow*)rows, *n_rows, tl, base, n, [](int64_t, int64_t) {});
    if (*hdr_bytes > hdr_cap) return CSV_OK;
    int64_t at = 0;
    fai_header_pieces((const FaiRow*)rows, *n_rows, tl, base, n, [&](int64_t s0, int64_t len) { memcpy(hdr + at, data + s0, (size_t)len); at += len; });
    return CSV_OK;
}

}  // extern "C"
