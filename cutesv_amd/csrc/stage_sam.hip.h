// stage_sam.hip.h — SAM text -> BAM file on the device (SamState in ctx.hip.h; sam_core.h; k_sam_* at the end of bam.hip.h; DESIGN.md
// section 41): csv_sam_to_bam and csv_sam_stats.  The text goes up window by window through the page-locked staging block; per window
// the marks, the plan, one scan, the two write kernels; the BAM stream stays in device memory and is compressed where it lies by
// stage_deflate.hip.h's dfl_run in blocks of SAM_BLOCK bytes - the header image is the prefix of the first window's stream, the bytes of
// a partial last block are carried in front of the next window's.  Down come the counts, the host items' line numbers, the patch rows
// and the compressed blocks; up go the text, the host items' records and the patch rows' answers.  Host code; included by
// cutesv_hip.hip behind stage_bam_sort.hip.h.

extern "C" __attribute__((visibility("hidden"))) void csv_sam_host_last(int64_t* counts, double* ms);

namespace {

// the refusal of a window: the serial rule over its lines from the first on names the lowest refused line (an error path: its cost does not matter)
int sam_refuse_window(csv_ctx* c, const uint8_t* t, i64 w0, i64 w1, i64 first_line, const SamNames& N)
{
    std::vector<uint8_t> rec;
    SamCounts cnt;
    i64 bad = 0;
    for (i64 a = w0; a < w1;) {                           // (line by line: the records are dropped as they come)
        const uint8_t* nl = (const uint8_t*)memchr(t + a, '\n', (size_t)(w1 - a));
        const i64 e = nl ? nl - t : w1;
        rec.clear();
        const int why = sam_line_record(t, a, e, N, &rec, &cnt);
        if (why) { bad = first_line + 1; return fail(c, CSV_E_INVALID, "%s", sam_refusal(bad, why).c_str()); }
        a = e + 1; first_line++;
    }
    return fail(c, CSV_E_HIP, "csv_sam_to_bam: the device refused a line the host rule takes");
}

// One window: text t[w0, w1) (whole lines; first_line: the 0-based ordinal of its first line in the file) -> its records behind the
// carried bytes (and `head`, the header image, in the first window) in s.stream; *stream_bytes: carried bytes, header and records
int sam_window(csv_ctx* c, const uint8_t* t, i64 w0, i64 w1, i64 first_line, const SamHeader& H, const uint8_t* head, i64 head_bytes, i64* n_lines_out, i64* stream_bytes)
{
    SamState& s = c->sam;
    hipStream_t st = c->stream;
    const bool add_nl = t[w1 - 1] != '\n';                 // (the file's last line without its line break: the window gets one)
    const i64 n = w1 - w0 + (add_nl ? 1 : 0);
    const int n_tiles = div_up(n, SAM_TILE);
    TRY(pin_reserve(c, (size_t)n + 64));
    memcpy(c->h_pin, t + w0, (size_t)(w1 - w0));
    if (add_nl) c->h_pin[n - 1] = '\n';
    memset(c->h_pin + n, 0, 64);
    TRY(reserve(c, s.text, (size_t)n + 64));
    TRY(reserve(c, s.cnt, (size_t)n_tiles * 8 * 4));
    TRY(reserve(c, s.small, 64));
    HIP_TRY(c, hipMemcpyAsync(s.text.p, c->h_pin, (size_t)n + 64, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(s.small.p, 0, 16, st));      // counters: host items, patch rows, CG records
    HIP_TRY(c, hipMemsetAsync((char*)s.small.p + 16, 0xff, 8, st));    // verdict
    s.st.up += n + 64;
    SamArgs A{};
    A.t = dp<uint8_t>(s.text); A.n = n;
    A.cnt_nl = dp<int>(s.cnt); A.cnt_tab = dp<int>(s.cnt) + (size_t)n_tiles * 4;
    A.counters = dp<int>(s.small); A.verdict = (u64*)((char*)s.small.p + 16);
    A.names = SamNames{dp<uint8_t>(s.names), (const int32_t*)((char*)s.names_tab.p), (const int32_t*)((char*)s.names_tab.p) + H.off.size(), (int32_t)H.id.size()};
    // the marks: counted, then written
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_sam_marks<false>, dim3(n_tiles), dim3(256), 0, st, A);
    HIP_TRY(c, hipGetLastError());
    s.cnt_h.resize((size_t)n_tiles * 8);
    HIP_TRY(c, hipMemcpyAsync(s.cnt_h.data(), s.cnt.p, (size_t)n_tiles * 8 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    s.st.down += (i64)n_tiles * 32;
    i64 n_lines = 0, n_tabs = 0;
    for (size_t k = 0; k < (size_t)n_tiles * 4; k++) { n_lines += s.cnt_h[k]; n_tabs += s.cnt_h[(size_t)n_tiles * 4 + k]; }
    if (n_lines < 1 || n_lines > (1ll << 31) - 8192) return fail(c, CSV_E_INVALID, "csv_sam_to_bam: a window of %lld lines", (long long)n_lines);
    const size_t z = (size_t)n_lines;
    const int n_dtile = div_up(n_lines, SORT_DST_TILE);
    TRY(reserve(c, s.nl, 8 * z));
    TRY(reserve(c, s.tab, 8 * (size_t)n_tabs + 8));
    TRY(reserve(c, s.rows, sizeof(SamRow) * z));
    TRY(reserve(c, s.len, 8 * z));
    TRY(reserve(c, s.dst, 8 * (z + 1)));
    TRY(reserve(c, s.tiles, 8 * (size_t)n_dtile));
    TRY(reserve(c, s.items, 4 * z));
    TRY(reserve(c, s.patches, sizeof(SamPatch) * ((size_t)n_tabs + 1)));
    A.nl = dp<i64>(s.nl); A.tab = dp<i64>(s.tab); A.n_lines = n_lines; A.n_tabs = n_tabs;
    A.rows = dp<SamRow>(s.rows); A.len = dp<i64>(s.len); A.dst = dp<i64>(s.dst); A.items = dp<int>(s.items);
    A.patches = dp<SamPatch>(s.patches); A.patch_cap = n_tabs + 1;
    hipLaunchKernelGGL(k_sam_marks<true>, dim3(n_tiles), dim3(256), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    hipLaunchKernelGGL(k_sam_plan, dim3(div_up(n_lines, 4)), dim3(256), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    HIP_TRY(c, hipGetLastError());
    int counters[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(counters, s.small.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); s.st.ms[0] += ms;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); s.st.ms[1] += ms;
    s.st.down += 8;
    // the host items: the serial rule on their lines; their records go up, their sizes into the plan
    const i64 n_items = counters[0];
    const SamNames N = H.table();
    const uint8_t* wt = (const uint8_t*)c->h_pin;          // the window as it went up
    SamCounts cnt;
    if (n_items < 0 || n_items > n_lines) return fail(c, CSV_E_HIP, "csv_sam_to_bam: %lld host items of %lld lines", (long long)n_items, (long long)n_lines);
    SamItemArgs I{};
    if (n_items > 0) {
        s.item_line.resize((size_t)n_items);
        HIP_TRY(c, hipMemcpyAsync(s.item_line.data(), s.items.p, 4 * (size_t)n_items, hipMemcpyDeviceToHost, st));
        // (a line's begin: the line break in front of it; those come down with the items - one gather would do, the whole list is simpler and small)
        s.nl_h.resize(z);
        HIP_TRY(c, hipMemcpyAsync(s.nl_h.data(), s.nl.p, 8 * z, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        s.st.down += 4 * n_items + 8 * n_lines;
        std::sort(s.item_line.begin(), s.item_line.end());
        s.item_rec.clear(); s.item_off.assign((size_t)n_items, 0); s.item_size.assign((size_t)n_items, 0);
        for (i64 k = 0; k < n_items; k++) {
            const i64 line = s.item_line[(size_t)k];
            if (line < 0 || line >= n_lines) return fail(c, CSV_E_HIP, "csv_sam_to_bam: a host item outside the window");
            const i64 b = line == 0 ? 0 : s.nl_h[(size_t)line - 1] + 1, e = s.nl_h[(size_t)line];
            if (b < 0 || e < b || e >= n) return fail(c, CSV_E_HIP, "csv_sam_to_bam: a line outside the window");
            const size_t at = s.item_rec.size();
            const int why = sam_line_record(wt, b, e, N, &s.item_rec, &cnt);
            if (why) return sam_refuse_window(c, t, w0, w1, first_line, N);
            s.item_off[(size_t)k] = (i64)at; s.item_size[(size_t)k] = (i64)(s.item_rec.size() - at);
        }
        const size_t zi = (size_t)n_items;
        TRY(reserve(c, s.item_tab, 20 * zi));
        TRY(reserve(c, s.item_bytes, s.item_rec.size() + 16));
        char* it = (char*)s.item_tab.p;
        HIP_TRY(c, hipMemcpyAsync(it, s.item_off.data(), 8 * zi, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(it + 8 * zi, s.item_size.data(), 8 * zi, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(it + 16 * zi, s.item_line.data(), 4 * zi, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(s.item_bytes.p, s.item_rec.data(), s.item_rec.size(), hipMemcpyHostToDevice, st));
        s.st.up += 20 * n_items + (i64)s.item_rec.size();
        I = SamItemArgs{(const int*)(it + 16 * zi), (const i64*)it, (const i64*)(it + 8 * zi), n_items, dp<uint8_t>(s.item_bytes), dp<i64>(s.len), dp<i64>(s.dst), nullptr, 0};
        hipLaunchKernelGGL(k_sam_item_len, dim3(div_up(n_items, 256)), dim3(256), 0, st, I);
    }
    // the sizes' exclusive scan, the total
    const SortDstArgs D{dp<i64>(s.len), nullptr, n_lines, dp<i64>(s.dst), dp<i64>(s.tiles)};
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_sort_dst_tiles, dim3(n_dtile), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sort_dst_scan, dim3(n_dtile), dim3(256), 0, st, D);
    HIP_TRY(c, hipGetLastError());
    i64 total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, dp<i64>(s.dst) + n_lines, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    s.st.down += 8;
    if (total < 36 * n_lines) return fail(c, CSV_E_HIP, "csv_sam_to_bam: %lld lines planned as %lld bytes", (long long)n_lines, (long long)total);
    // the stream buffer: the carried bytes, the header image (first window), the records
    const i64 base = s.carry_bytes + head_bytes;
    TRY(reserve(c, s.stream, (size_t)(base + total) + 64));
    if (s.carry_bytes > 0) HIP_TRY(c, hipMemcpyAsync(s.stream.p, s.carry.p, (size_t)s.carry_bytes, hipMemcpyDeviceToDevice, st));
    if (head_bytes > 0) { HIP_TRY(c, hipMemcpyAsync((char*)s.stream.p + s.carry_bytes, head, (size_t)head_bytes, hipMemcpyHostToDevice, st)); s.st.up += head_bytes; }
    A.out = dp<uint8_t>(s.stream); A.base = base; A.total = total;
    hipLaunchKernelGGL(k_sam_small, dim3(div_up(n_lines, 4)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_sam_bulk, dim3(div_up(div_up(base + total, SAM_BULK_TILE), 4)), dim3(256), 0, st, A);
    if (n_items > 0) {
        I.out = A.out; I.base = base;
        hipLaunchKernelGGL(k_sam_items, dim3(div_up(n_items, 4)), dim3(256), 0, st, I);
    }
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    u64 small[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(small, s.small.p, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); s.st.ms[2] += ms;
    s.st.down += 24;
    if (small[2] != ~0ull) return sam_refuse_window(c, t, w0, w1, first_line, N);
    // the patch rows: strtod on the host, four bytes each back up
    const i64 n_patch = (i64)(small[0] >> 32);
    if (n_patch < 0 || n_patch > A.patch_cap) return fail(c, CSV_E_HIP, "csv_sam_to_bam: %lld patch rows", (long long)n_patch);
    if (n_patch > 0) {
        std::vector<SamPatch> P((size_t)n_patch);
        std::vector<uint32_t> bits((size_t)n_patch);
        HIP_TRY(c, hipMemcpyAsync(P.data(), s.patches.p, sizeof(SamPatch) * (size_t)n_patch, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        for (i64 k = 0; k < n_patch; k++) {
            const SamPatch& p = P[(size_t)k];
            if (p.text_off < 0 || p.len < 1 || p.len > SAM_NUM_MAX || p.text_off > n - p.len || p.out_off < base || p.out_off > base + total - 4)
                return fail(c, CSV_E_HIP, "csv_sam_to_bam: a patch row outside the window");
            const std::string txt((const char*)wt + p.text_off, (size_t)p.len);
            char* end = nullptr;
            const double d = strtod(txt.c_str(), &end);    // (the device's grammar holds: strtod takes all of it)
            bits[(size_t)k] = sam_float_bits((float)d);
        }
        TRY(reserve(c, s.patch_bits, 4 * (size_t)n_patch));
        HIP_TRY(c, hipMemcpyAsync(s.patch_bits.p, bits.data(), 4 * (size_t)n_patch, hipMemcpyHostToDevice, st));
        // (the rows went down in atomic order and are used in that order: row k and answer k belong together)
        hipLaunchKernelGGL(k_sam_patch, dim3(div_up(n_patch, 256)), dim3(256), 0, st, (const SamPatch*)dp<SamPatch>(s.patches), (const uint32_t*)dp<uint32_t>(s.patch_bits), n_patch,
                           dp<uint8_t>(s.stream));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(st));
        s.st.down += (i64)sizeof(SamPatch) * n_patch; s.st.up += 4 * n_patch;
    }
    s.st.patches += n_patch + cnt.patches;
    s.st.cg += cnt.cg + (i64)(small[1] & 0xffffffffull);
    *n_lines_out = n_lines; *stream_bytes = base + total;
    return CSV_OK;
}

}  // namespace

extern "C" {

int csv_sam_to_bam(csv_ctx* c, const char* sam_path, const char* out_path, int64_t window_bytes, int32_t flags)
{
    if (!c) return CSV_E_INVALID;
    SamState& s = c->sam;
    s.st = SamStats();
    if (!sam_path || !out_path || window_bytes < 0 || window_bytes > SAM_WINDOW_MAX || flags != 0) return fail(c, CSV_E_INVALID, "bad csv_sam_to_bam");
    if (window_bytes == 0) window_bytes = SAM_WINDOW;
    SamMap M;
    std::string text;
    if (!M.open(sam_path, &text)) return fail(c, CSV_E_INVALID, "%s", text.c_str());
    SamHeader H;
    if (!sam_header_parse(M.t, M.n, &H, &text)) return fail(c, CSV_E_INVALID, "%s", text.c_str());
    SamStats& st = s.st;
    st.header_bytes = (i64)H.image.size(); st.text_bytes = M.n; st.lines = H.lines;
    HIP_TRY(c, hipSetDevice(c->device));
    // the name table
    TRY(reserve(c, s.names, H.blob.size() + 64));
    TRY(reserve(c, s.names_tab, 4 * (H.off.size() + H.id.size()) + 16));
    TRY(reserve(c, s.carry, (size_t)SAM_BLOCK + 64));
    TRY(h2d(c, s.names, H.blob.data(), (i64)H.blob.size()));
    HIP_TRY(c, hipMemcpyAsync(s.names_tab.p, H.off.data(), 4 * H.off.size(), hipMemcpyHostToDevice, c->stream));
    if (!H.id.empty()) HIP_TRY(c, hipMemcpyAsync((char*)s.names_tab.p + 4 * H.off.size(), H.id.data(), 4 * H.id.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    st.up += (i64)(H.blob.size() + 4 * (H.off.size() + H.id.size()));
    s.carry_bytes = 0;
    FILE* f = nullptr;
    auto finish = [&](int rc) {
        if (f) fclose(f);
        if (rc && f) remove(out_path);
        return rc;
    };
    std::vector<uint8_t> image;
    std::vector<int32_t> sizes;
    std::vector<i64> off;
    std::vector<int32_t> ln;
    // `len` bytes at the front of the stream buffer (dev, or the host's `host` when nothing lies on the device) -> blocks into the file
    auto deflate = [&](const uint8_t* host, i64 len) -> int {
        const int32_t nb = (int32_t)((len + SAM_BLOCK - 1) / SAM_BLOCK);
        if (nb == 0) return CSV_OK;
        off.resize((size_t)nb); ln.resize((size_t)nb); sizes.resize((size_t)nb);
        for (int32_t k = 0; k < nb; k++) { off[(size_t)k] = (i64)k * SAM_BLOCK; ln[(size_t)k] = (int32_t)std::min<i64>(SAM_BLOCK, len - (i64)k * SAM_BLOCK); }
        image.resize((size_t)(len + 31ll * nb));
        int64_t out_bytes = 0;
        double ms_d = 0;
        static_assert(sizeof(i64) == sizeof(int64_t), "the block table is handed on as it is");
        TRY(dfl_run(c, host ? nullptr : dp<uint8_t>(s.stream), host, len, nb, (const int64_t*)off.data(), ln.data(), image.data(), (int64_t)image.size(), sizes.data(), &out_bytes, &ms_d));
        if (out_bytes <= 0 || out_bytes > (int64_t)image.size()) return fail(c, CSV_E_HIP, "csv_sam_to_bam: the stream compressed to nothing");
        if (!f && !(f = fopen(out_path, "wb"))) return fail(c, CSV_E_INVALID, "cannot write %s", out_path);
        if (fwrite(image.data(), 1, (size_t)out_bytes, f) != (size_t)out_bytes) return fail(c, CSV_E_INVALID, "cannot write %s", out_path);
        st.ms[3] += ms_d; st.blocks += nb; st.out_bytes += out_bytes; st.stream_bytes += len;
        st.up += 12ll * nb + (host ? len : 0); st.down += out_bytes + 4ll * nb + 8;
        return CSV_OK;
    };
    bool first = true;
    for (i64 w0 = H.text_bytes; w0 < M.n;) {
        const i64 w1 = sam_window_end(M.t, M.n, w0, window_bytes);
        if (w1 - w0 >= SAM_WINDOW_MAX) return finish(fail(c, CSV_E_INVALID, "%s", sam_refusal(st.lines + 1, SAM_E_SIZE).c_str()));
        i64 n_lines = 0, bytes = 0;
        int rc = sam_window(c, M.t, w0, w1, st.lines, H, first ? H.image.data() : nullptr, first ? (i64)H.image.size() : 0, &n_lines, &bytes);
        if (rc) return finish(rc);
        first = false;
        st.lines += n_lines; st.records += n_lines; st.windows++;
        w0 = w1;
        const bool last = w0 >= M.n;
        const i64 len = last ? bytes : bytes / SAM_BLOCK * SAM_BLOCK;
        if ((rc = deflate(nullptr, len)) != CSV_OK) return finish(rc);
        s.carry_bytes = bytes - len;
        if (s.carry_bytes > 0) {
            HIP_TRY(c, hipMemcpyAsync(s.carry.p, (char*)s.stream.p + len, (size_t)s.carry_bytes, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    if (first) {                                             // no alignment line: the header image alone
        const int rc = deflate(H.image.data(), (i64)H.image.size());
        if (rc) return finish(rc);
    }
    if (fwrite(SAM_EOF_BLOCK, 1, sizeof SAM_EOF_BLOCK, f) != sizeof SAM_EOF_BLOCK) return finish(fail(c, CSV_E_INVALID, "cannot write %s", out_path));
    st.blocks++; st.out_bytes += (i64)sizeof SAM_EOF_BLOCK;
    return finish(CSV_OK);
}

int csv_sam_stats(const csv_ctx* c, int64_t* counts, double* ms)
{
    if (c) sam_stats_out(c->sam.st, counts, ms);
    else csv_sam_host_last(counts, ms);
    return CSV_OK;
}

}  // extern "C"
