// stage_inflate.hip.h — csv_bgzf_inflate: the raw-deflate payloads of BGZF blocks -> their bytes, one wavefront per block
// (k_bgzf_inflate at the end of bam.hip.h over inflate_core.h).  The device buffers are InflateState's own
// (ctx.hip.h): no arena is planned, no generation word moves, and nothing another stage left on the device is touched.
// Host code; included by cutesv_hip.hip behind stage_bam.hip.h.

// csv_bgzf_inflate, and its internal form (dev_out != NULL; stage_frame.hip.h): the bytes are written to dev_out - device memory of
// out_bytes bytes - and stay there; `out` is not touched.  The checks, the tables and the status bytes are the same.
static int inflate_impl(csv_ctx* c, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                        const int32_t* out_len, const uint32_t* crc, uint8_t* out, uint8_t* dev_out, int64_t out_bytes, int32_t flags, uint8_t* status, double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (ms_kernels) *ms_kernels = 0;
    if (n_blocks < 0 || comp_bytes < 0 || out_bytes < 0 || flags != 0) return fail(c, CSV_E_INVALID, "bad bgzf inflate");
    if (n_blocks == 0) return CSV_OK;
    if (!in_off || !in_len || !out_off || !out_len || !crc || !status || (comp_bytes > 0 && !comp) || (out_bytes > 0 && !out && !dev_out)) return fail(c, CSV_E_INVALID, "bad bgzf inflate");
    InflateState& s = c->inf;
    // every range is checked before anything is launched: the kernel trusts them
    s.order.clear();
    bool sorted = true;
    for (int32_t k = 0; k < n_blocks; k++) {
        if (in_len[k] < 0 || in_off[k] < 0 || in_off[k] > comp_bytes - in_len[k])
            return fail(c, CSV_E_INVALID, "csv_bgzf_inflate: the payload of block %d lies outside comp", (int)k);
        if (out_len[k] < 0 || out_len[k] > 65536) return fail(c, CSV_E_INVALID, "csv_bgzf_inflate: out_len of block %d is %d (0 .. 65536)", (int)k, (int)out_len[k]);
        if (out_off[k] < 0 || out_off[k] > out_bytes - out_len[k]) return fail(c, CSV_E_INVALID, "csv_bgzf_inflate: the output of block %d lies outside out", (int)k);
        if (out_len[k] == 0) continue;
        if (!s.order.empty() && out_off[s.order.back()] > out_off[k]) sorted = false;
        s.order.push_back(k);
    }
    if (!sorted) std::sort(s.order.begin(), s.order.end(), [&](int32_t x, int32_t y) { return out_off[x] < out_off[y]; });
    for (size_t i = 1; i < s.order.size(); i++)
        if (out_off[s.order[i - 1]] + out_len[s.order[i - 1]] > out_off[s.order[i]])
            return fail(c, CSV_E_INVALID, "csv_bgzf_inflate: the outputs of blocks %d and %d overlap", (int)s.order[i - 1], (int)s.order[i]);
    memset(status, 0, (size_t)n_blocks);
    if (s.order.empty()) return CSV_OK;                            // nothing but empty blocks
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // tab: in_off, out_off (8 bytes each), then in_len, out_len, crc (4 each), per block
    const size_t n = (size_t)n_blocks, o_out_off = 8 * n, o_in_len = 16 * n, o_out_len = 20 * n, o_crc = 24 * n;
    s.tab_h.resize(28 * n);
    memcpy(s.tab_h.data(), in_off, 8 * n); memcpy(s.tab_h.data() + o_out_off, out_off, 8 * n);
    memcpy(s.tab_h.data() + o_in_len, in_len, 4 * n); memcpy(s.tab_h.data() + o_out_len, out_len, 4 * n); memcpy(s.tab_h.data() + o_crc, crc, 4 * n);
    TRY(reserve(c, s.comp, (size_t)comp_bytes + 8));
    TRY(reserve(c, s.tab, 28 * n));
    if (!dev_out) TRY(reserve(c, s.out, (size_t)out_bytes + 8));
    TRY(reserve(c, s.status, n));
    TRY(h2d(c, s.comp, comp, comp_bytes));
    TRY(h2d(c, s.tab, s.tab_h.data(), (i64)(28 * n)));
    char* t = (char*)s.tab.p;
    const InflateArgs A{(int)n_blocks, dp<uint8_t>(s.comp), (const i64*)t, (const int*)(t + o_in_len), (const i64*)(t + o_out_off), (const int*)(t + o_out_len),
                        (const unsigned*)(t + o_crc), dev_out ? dev_out : dp<uint8_t>(s.out), dp<uint8_t>(s.status)};
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(std::min(div_up(n_blocks, INF_WAVES), 8192)), dim3(64 * INF_WAVES), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    // the bytes come back in runs of adjacent outputs (a reader's window: one run), so that no byte of `out` between two blocks is written
    for (size_t i = 0; !dev_out && i < s.order.size();) {
        size_t j = i + 1;
        while (j < s.order.size() && out_off[s.order[j - 1]] + out_len[s.order[j - 1]] == out_off[s.order[j]]) j++;
        const int64_t b0 = out_off[s.order[i]], b1 = out_off[s.order[j - 1]] + out_len[s.order[j - 1]];
        HIP_TRY(c, hipMemcpyAsync(out + b0, dp<uint8_t>(s.out) + b0, (size_t)(b1 - b0), hipMemcpyDeviceToHost, st));
        i = j;
    }
    HIP_TRY(c, hipMemcpyAsync(status, s.status.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (ms_kernels) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        *ms_kernels = ms;
    }
    return CSV_OK;
}

extern "C" {

int csv_bgzf_inflate(csv_ctx* c, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                     const int32_t* out_len, const uint32_t* crc, uint8_t* out, int64_t out_bytes, int32_t flags, uint8_t* status, double* ms_kernels)
{
    return inflate_impl(c, comp, comp_bytes, n_blocks, in_off, in_len, out_off, out_len, crc, out, nullptr, out_bytes, flags, status, ms_kernels);
}

}  // extern "C"
