// stage_frame.hip.h — record framing on the device (FrameState in ctx.hip.h; frame_core.h; k_frame_* at the end of bam.hip.h;
// DESIGN.md section 29): the reader's internal entries (csv_frame_*, declared in frame_core.h, called by bam_host.cpp) and the three
// consumers of a device chunk.  The inflated window, the slim image and the host image stay in device memory; what comes down is
// the row table, what goes up are block tables, pack tables and the blocks the host had to inflate.  Host code; included by
// cutesv_hip.hip behind stage_inflate.hip.h.

// the next window: `bytes` bytes, of which the first `keep` are [keep_at, keep_at + keep) of the current one - copied into the other
// buffer, so no copy overlaps - and the rest are the n_blocks blocks given, inflated in place (out_off counts from the window's start)
int csv_frame_window(csv_ctx* c, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                     const int32_t* out_len, const uint32_t* crc, int64_t bytes, int64_t keep, int64_t keep_at, uint8_t* status, double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (ms_kernels) *ms_kernels = 0;
    if (bytes < 0 || keep < 0 || keep > bytes || (keep > 0 && (keep_at < 0 || keep_at > f.win_n - keep))) return fail(c, CSV_E_INVALID, "bad frame window");
    HIP_TRY(c, hipSetDevice(c->device));
    const int nx = f.cur ^ 1;
    TRY(reserve(c, f.win[nx], (size_t)bytes + 16));
    if (keep > 0) HIP_TRY(c, hipMemcpyAsync(f.win[nx].p, dp<uint8_t>(f.win[f.cur]) + keep_at, (size_t)keep, hipMemcpyDeviceToDevice, c->stream));
    for (int32_t k = 0; k < n_blocks; k++)                                   // (the kept bytes are not written again)
        if (out_off[k] < keep) return fail(c, CSV_E_INVALID, "bad frame window: block %d lies in the kept bytes", (int)k);
    if (n_blocks > 0) TRY(inflate_impl(c, comp, comp_bytes, n_blocks, in_off, in_len, out_off, out_len, crc, nullptr, dp<uint8_t>(f.win[nx]), bytes, 0, status, ms_kernels));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    f.cur = nx; f.win_n = bytes; f.serial++; f.n_rows = 0;
    f.bytes_up += comp_bytes + 28ll * n_blocks; f.bytes_down += n_blocks;
    return CSV_OK;
}

uint64_t csv_frame_window_serial(const csv_ctx* c) { return c ? c->fr.serial : 0; }

int csv_frame_window_put(csv_ctx* c, int64_t off, const uint8_t* src, int64_t len)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (off < 0 || len < 0 || off > f.win_n - len || (len > 0 && !src)) return fail(c, CSV_E_INVALID, "bad frame window block");
    if (len == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dp<uint8_t>(f.win[f.cur]) + off, src, (size_t)len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    f.bytes_up += len;
    return CSV_OK;
}

// frame the current window from `cursor` (a true record start): *rows = one row per framed record (host memory of the state, valid
// until the next call), *res = where the chain stopped.  rows == NULL: the rows stay in device memory (FrameState::rows, for
// csv_index_window) and do not come down
int csv_frame_run(csv_ctx* c, int32_t n_blocks, const int64_t* blk_off, const int32_t* blk_len, int32_t n_ref, int64_t cursor, const FrRow** rows, FrStitch* res)
{
    if (!c || !res) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (rows) *rows = nullptr;
    f.n_rows = 0;
    if (n_blocks < 1 || !blk_off || !blk_len || cursor < 0 || cursor > f.win_n) return fail(c, CSV_E_INVALID, "bad frame call");
    // the table is checked before anything is launched: the kernels trust it (contiguous from 0 to the window's end)
    const size_t n = (size_t)n_blocks;
    const size_t o_slot = 8 * n, o_len = 16 * n, o_g = (20 * n + 15) & ~(size_t)15, o_ex = o_g + 8 * n, o_cnt = o_ex + 8 * n, o_used = o_cnt + 4 * n;
    const size_t o_scan = (o_used + 4 * n + 15) & ~(size_t)15, o_tile = o_scan + 16 * n, o_tot = o_tile + scan_tile_bytes(n_blocks), o_res = o_tot + 24, total = o_res + sizeof(FrStitch);
    f.tab_h.resize(o_g);
    i64* h_off = (i64*)f.tab_h.data(); i64* h_slot = (i64*)(f.tab_h.data() + o_slot); int32_t* h_len = (int32_t*)(f.tab_h.data() + o_len);
    i64 at = 0, slots = 0;
    for (size_t s = 0; s < n; s++) {
        if (blk_off[s] != at || blk_len[s] < 0 || blk_len[s] > 65536) return fail(c, CSV_E_INVALID, "bad frame call: block %d of the table", (int)s);
        h_off[s] = at; h_len[s] = blk_len[s]; h_slot[s] = slots;
        at += blk_len[s]; slots += fr_slot_size(blk_len[s]);
    }
    if (at != f.win_n) return fail(c, CSV_E_INVALID, "bad frame call: the block table covers %lld of the window's %lld bytes", (long long)at, (long long)f.win_n);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TRY(reserve(c, f.tab, total));
    TRY(reserve(c, f.starts, (size_t)slots * 8 + 16));
    TRY(h2d(c, f.tab, f.tab_h.data(), (i64)o_g));
    char* t = (char*)f.tab.p;
    FrameArgs A{};
    A.W = FrWin{dp<uint8_t>(f.win[f.cur]), f.win_n, n_ref}; A.n_blocks = n_blocks; A.c = cursor;
    A.blk_off = (const i64*)t; A.slot_off = (const i64*)(t + o_slot); A.blk_len = (const int*)(t + o_len);
    A.g = (i64*)(t + o_g); A.ex = (i64*)(t + o_ex); A.cnt = (int*)(t + o_cnt); A.used = (int*)(t + o_used); A.scan = (int4*)(t + o_scan);
    A.starts = dp<i64>(f.starts); A.res = (FrStitch*)(t + o_res); A.rows = nullptr;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_frame_guess, dim3(std::min(div_up(n_blocks, FRAME_WAVES), 8192)), dim3(64 * FRAME_WAVES), 0, st, A);
    hipLaunchKernelGGL(k_frame_stitch, dim3(1), dim3(64), 0, st, A);
    scan_counts(st, ScanArgs{n_blocks, A.scan, (i64*)(t + o_tile), (i64*)(t + o_tot)});
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    FrStitch R;
    HIP_TRY(c, hipMemcpyAsync(&R, A.res, sizeof R, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (R.n_records < 0 || R.n_records > slots || R.tail < cursor || R.tail > f.win_n) return fail(c, CSV_E_INVALID, "frame: inconsistent counts (%lld records)", (long long)R.n_records);
    float ms = 0, ms2 = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    f.rows_h.resize(rows ? (size_t)R.n_records : 0);
    if (R.n_records > 0) {
        TRY(reserve(c, f.rows, (size_t)R.n_records * sizeof(FrRow)));
        A.rows = dp<FrRow>(f.rows);
        HIP_TRY(c, hipEventRecord(c->ev[2], st));
        hipLaunchKernelGGL(k_frame_rows, dim3(std::min(div_up(n_blocks, FRAME_WAVES), 8192)), dim3(64 * FRAME_WAVES), 0, st, A, (i64)R.n_records);
        HIP_TRY(c, hipEventRecord(c->ev[3], st));
        HIP_TRY(c, hipGetLastError());
        if (rows) HIP_TRY(c, hipMemcpyAsync(f.rows_h.data(), f.rows.p, (size_t)R.n_records * sizeof(FrRow), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        HIP_TRY(c, hipEventElapsedTime(&ms2, c->ev[2], c->ev[3]));
    }
    f.ms_kernels += ms + ms2;
    f.right += R.right_blocks; f.fallback += R.fallback_blocks;
    f.bytes_up += (i64)o_g; f.bytes_down += (i64)sizeof R + (rows ? R.n_records * (i64)sizeof(FrRow) : 0);
    f.n_rows = R.n_records;
    if (rows) *rows = f.rows_h.data();
    *res = R;
    return CSV_OK;
}

int csv_frame_chunk_begin(csv_ctx* c, const void* owner)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    f.owner = owner; f.chunk_ok = false;
    f.n = 0; f.slim_bytes = 0; f.host_bytes = 0;
    return CSV_OK;
}

// n selected records of the current window into the images, which hold slim_bytes / host_bytes bytes afterwards
int csv_frame_pack(csv_ctx* c, int64_t n, const FrPack* p, int64_t slim_bytes, int64_t host_bytes)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (n < 0 || (n > 0 && !p) || slim_bytes < f.slim_bytes || host_bytes < f.host_bytes) return fail(c, CSV_E_INVALID, "bad frame pack");
    if (n == 0) return CSV_OK;
    // every source and destination range is checked before the kernel runs: it trusts the table
    for (i64 r = 0; r < n; r++) {
        const FrPack& q = p[r];
        const FrLayout y = fr_layout(q.bs, q.l_name, q.n_cig, q.l_seq);
        if (q.bs < 32 || y.fixed_to_aux > q.bs || q.src < 0 || q.src > f.win_n - 4 - (i64)q.bs || q.rec_off < f.slim_bytes || (q.rec_off & 15) || q.rec_off > slim_bytes - y.slim_padded ||
            q.host_off < f.host_bytes || q.host_off > host_bytes - y.host_len)
            return fail(c, CSV_E_INVALID, "bad frame pack: record %lld leaves the window or the images", (long long)r);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(grow_keep(c, f.slim, (size_t)slim_bytes + 16, (size_t)f.slim_bytes));
    TRY(grow_keep(c, f.host, (size_t)host_bytes + 16, (size_t)f.host_bytes));
    TRY(reserve(c, f.pack, (size_t)n * sizeof(FrPack)));
    hipStream_t st = c->stream;
    TRY(h2d(c, f.pack, p, n * (i64)sizeof(FrPack)));
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_frame_pack, dim3(std::min(div_up(n, 4), 8192)), dim3(256), 0, st, dp<uint8_t>(f.win[f.cur]), dp<FrPack>(f.pack), (i64)n, dp<uint8_t>(f.slim), dp<uint8_t>(f.host));
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    f.ms_kernels += ms;
    f.bytes_up += n * (i64)sizeof(FrPack);
    f.slim_bytes = slim_bytes; f.host_bytes = host_bytes;
    return CSV_OK;
}

int csv_frame_chunk_end(csv_ctx* c, int64_t n, const int64_t* rec_off, const uint32_t* rec_len, const int64_t* host_off, const int32_t* l_name, const int32_t* l_seq)
{
    if (!c || n < 0 || (n > 0 && (!rec_off || !rec_len || !host_off || !l_name || !l_seq))) return CSV_E_INVALID;
    FrameState& f = c->fr;
    f.rec_off.assign(rec_off, rec_off + n); f.rec_len.assign(rec_len, rec_len + n); f.host_off.assign(host_off, host_off + n);
    f.l_name.assign(l_name, l_name + n); f.l_seq.assign(l_seq, l_seq + n);
    f.n = n; f.chunk_ok = true;
    return CSV_OK;
}

// one framing reader per context: the window, the chunk and the *_framed consumers are the context's, so a second reader would
// hand its images to the first one's consumers
int csv_frame_reader(csv_ctx* c, const void* owner, int set)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (set) {
        if (f.reader && f.reader != owner) return CSV_E_STATE;
        f.reader = owner;
        return CSV_OK;
    }
    if (f.reader == owner) f.reader = nullptr;
    if (f.owner == owner) { f.chunk_ok = false; f.owner = nullptr; }
    return CSV_OK;
}

int csv_frame_fetch(csv_ctx* c, const void* owner, uint8_t* slim, uint8_t* host)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (!f.chunk_ok || f.owner != owner) return fail(c, CSV_E_STATE, "the context holds no valid device chunk of this reader (it lives until the reader's next read or route change)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (slim && f.slim_bytes > 0) HIP_TRY(c, hipMemcpyAsync(slim, f.slim.p, (size_t)f.slim_bytes, hipMemcpyDeviceToHost, c->stream));
    if (host && f.host_bytes > 0) HIP_TRY(c, hipMemcpyAsync(host, f.host.p, (size_t)f.host_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    f.bytes_down += (slim ? f.slim_bytes : 0) + (host ? f.host_bytes : 0);
    return CSV_OK;
}

int csv_frame_counters(csv_ctx* c, int64_t* right, int64_t* fallback, double* ms_kernels, int64_t* bytes_down, int64_t* bytes_up, int reset)
{
    if (!c) return CSV_E_INVALID;
    FrameState& f = c->fr;
    if (right) *right = f.right;
    if (fallback) *fallback = f.fallback;
    if (ms_kernels) *ms_kernels = f.ms_kernels;
    if (bytes_down) *bytes_down = f.bytes_down;
    if (bytes_up) *bytes_up = f.bytes_up;
    if (reset) { f.right = f.fallback = f.bytes_down = f.bytes_up = 0; f.ms_kernels = 0; }
    return CSV_OK;
}

extern "C" {

static int frame_chunk_check(csv_ctx* c, const char* what)
{
    if (!c->fr.chunk_ok) return fail(c, CSV_E_STATE, "%s: the context holds no valid device chunk (csv_bam_set_frame; it lives until the reader's next read or route change)", what);
    return CSV_OK;
}

int csv_bam_decode_framed(csv_ctx* c, csv_bam_out* out)
{
    if (!c || !out) return CSV_E_INVALID;
    TRY(frame_chunk_check(c, "csv_bam_decode_framed"));
    FrameState& f = c->fr;
    csv_bam_in in{};
    in.n_records = f.n; in.slim = nullptr; in.slim_bytes = f.slim_bytes; in.rec_off = f.rec_off.data(); in.rec_len = f.rec_len.data(); in.flags = 0;
    return bam_decode_impl(c, &in, out, f.n > 0 ? dp<uint8_t>(f.slim) : nullptr);
}

int csv_name_pool_append_framed(csv_ctx* c, int64_t* first_index)
{
    if (!c) return CSV_E_INVALID;
    TRY(frame_chunk_check(c, "csv_name_pool_append_framed"));
    FrameState& f = c->fr;
    std::vector<int32_t> len((size_t)f.n);
    for (i64 i = 0; i < f.n; i++) len[(size_t)i] = f.l_name[(size_t)i] > 0 ? f.l_name[(size_t)i] - 1 : 0;
    return name_pool_append_impl(c, f.n, nullptr, dp<uint8_t>(f.host), f.host_bytes, f.host_off.data(), len.data(), first_index);
}

int csv_seq_reads_framed(csv_ctx* c, const uint8_t* want)
{
    if (!c) return CSV_E_INVALID;
    TRY(frame_chunk_check(c, "csv_seq_reads_framed"));
    FrameState& f = c->fr;
    std::vector<int64_t> off((size_t)f.n);
    for (i64 i = 0; i < f.n; i++) off[(size_t)i] = f.host_off[(size_t)i] + f.l_name[(size_t)i];
    return seq_reads_upload_impl(c, f.n, nullptr, dp<uint8_t>(f.host), f.host_bytes, off.data(), f.l_seq.data(), want);
}

}  // extern "C"
