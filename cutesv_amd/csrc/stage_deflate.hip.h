// stage_deflate.hip.h — csv_bgzf_deflate: blocks of at most 65280 bytes -> complete BGZF blocks packed into a file image, one wavefront
// per block (k_bgzf_deflate and k_deflate_offsets at the end of bam.hip.h over deflate_core.h, then k_frame_gather; DESIGN.md section
// 34).  The device buffers are DeflateState's own (ctx.hip.h): no arena is planned, no generation word moves, and nothing another
// stage left on the device is touched.  Host code; included by cutesv_hip.hip behind stage_inflate.hip.h.

// The body of both entries.  dev_in: the input where it already lies in device memory (csv_bgzf_deflate_text: the kept VCF text), or
// NULL: `in` is uploaded into DeflateState::in first (csv_bgzf_deflate).
static int dfl_run(csv_ctx* c, const uint8_t* dev_in, const uint8_t* in, int64_t in_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, uint8_t* out, int64_t out_cap,
                   int32_t* block_bytes, int64_t* out_bytes, double* ms_kernels)
{
    // every range is checked before anything is launched: the kernel trusts them
    for (int32_t k = 0; k < n_blocks; k++) {
        if (in_len[k] < 0 || in_len[k] > DFL_MAX_IN) return fail(c, CSV_E_INVALID, "csv_bgzf_deflate: in_len of block %d is %d (0 .. %d)", (int)k, (int)in_len[k], DFL_MAX_IN);
        if (in_off[k] < 0 || in_off[k] > in_bytes - in_len[k]) return fail(c, CSV_E_INVALID, "csv_bgzf_deflate: the input of block %d lies outside in", (int)k);
    }
    *out_bytes = 0;
    if (n_blocks == 0) return CSV_OK;
    DeflateState& s = c->dfl;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_blocks;
    const int grid = std::min(div_up(n_blocks, DFL_WAVES), 2 * c->n_cu);
    i64 bound = 0;                                                 // of the image: no block is larger than its stored form
    for (int32_t k = 0; k < n_blocks; k++) bound += in_len[k] + 31;
    // tab: in_off (8 bytes per block), then in_len (4); offs: the slot offsets, the image offsets (8 each), the total
    s.tab_h.resize(12 * n);
    memcpy(s.tab_h.data(), in_off, 8 * n); memcpy(s.tab_h.data() + 8 * n, in_len, 4 * n);
    if (!dev_in) TRY(reserve(c, s.in, (size_t)in_bytes + 8));
    TRY(reserve(c, s.tab, 12 * n));
    TRY(reserve(c, s.slots, n * (size_t)DFL_SLOT));
    TRY(reserve(c, s.tok, (size_t)grid * DFL_WAVES * DFL_MAX_IN * 4));
    TRY(reserve(c, s.size, 4 * n));
    TRY(reserve(c, s.offs, 16 * n + 8));
    TRY(reserve(c, s.image, (size_t)bound + 8));
    if (!dev_in) TRY(h2d(c, s.in, in, in_bytes));
    TRY(h2d(c, s.tab, s.tab_h.data(), (i64)(12 * n)));
    char* t = (char*)s.tab.p;
    i64* offs = dp<i64>(s.offs);
    const DeflateArgs A{(int)n_blocks, dev_in ? dev_in : dp<uint8_t>(s.in), (const i64*)t, (const int*)(t + 8 * n), dp<uint8_t>(s.slots), dp<uint32_t>(s.tok), dp<int>(s.size)};
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(64 * DFL_WAVES), 0, st, A);
    hipLaunchKernelGGL(k_deflate_offsets, dim3(1), dim3(256), 0, st, (const int*)dp<int>(s.size), (i64)n_blocks, offs, offs + n, offs + 2 * n);
    hipLaunchKernelGGL(k_frame_gather, dim3(std::min(div_up(n_blocks, 4), 8192)), dim3(256), 0, st, (const uint8_t*)dp<uint8_t>(s.slots), (const i64*)offs, (const int*)dp<int>(s.size), (i64)n_blocks,
                       dp<uint8_t>(s.image), (const i64*)(offs + n));
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    i64 total = 0;
    HIP_TRY(c, hipMemcpyAsync(block_bytes, s.size.p, 4 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&total, offs + 2 * n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (total < 0 || total > bound) return fail(c, CSV_E_HIP, "csv_bgzf_deflate: the image has %lld bytes, beyond its bound of %lld", (long long)total, (long long)bound);
    *out_bytes = total;
    if (total <= out_cap && total > 0) {                           // else: the caller learns the need, `out` stays as it is
        HIP_TRY(c, hipMemcpyAsync(out, s.image.p, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    if (ms_kernels) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        *ms_kernels = ms;
    }
    return CSV_OK;
}

extern "C" {

int csv_bgzf_deflate(csv_ctx* c, const uint8_t* in, int64_t in_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, uint8_t* out, int64_t out_cap,
                     int32_t* block_bytes, int64_t* out_bytes, int32_t flags, double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (ms_kernels) *ms_kernels = 0;
    if (n_blocks < 0 || in_bytes < 0 || out_cap < 0 || flags != 0 || !out_bytes) return fail(c, CSV_E_INVALID, "bad bgzf deflate");
    if (n_blocks > 0 && (!in_off || !in_len || !block_bytes || (in_bytes > 0 && !in) || (out_cap > 0 && !out))) return fail(c, CSV_E_INVALID, "bad bgzf deflate");
    return dfl_run(c, nullptr, in, in_bytes, n_blocks, in_off, in_len, out, out_cap, block_bytes, out_bytes, ms_kernels);
}

// csv_bgzf_deflate with the context's kept VCF text (csv_vcf_emit_device with CSV_VCF_KEEP_TEXT) as its input: the text is compressed
// where it lies.  Contract, cut rule and bytes are csv_bgzf_deflate's; CSV_E_INVALID also when the context keeps no text.
int csv_bgzf_deflate_text(csv_ctx* c, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, uint8_t* out, int64_t out_cap, int32_t* block_bytes, int64_t* out_bytes,
                          double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (ms_kernels) *ms_kernels = 0;
    if (n_blocks < 0 || out_cap < 0 || !out_bytes) return fail(c, CSV_E_INVALID, "bad bgzf deflate");
    if (n_blocks > 0 && (!in_off || !in_len || !block_bytes || (out_cap > 0 && !out))) return fail(c, CSV_E_INVALID, "bad bgzf deflate");
    if (!c->ve.kept) return fail(c, CSV_E_INVALID, "csv_bgzf_deflate_text: the context keeps no VCF text (csv_vcf_emit_device with CSV_VCF_KEEP_TEXT)");
    return dfl_run(c, dp<uint8_t>(c->ve.text), nullptr, c->ve.text_bytes, n_blocks, in_off, in_len, out, out_cap, block_bytes, out_bytes, ms_kernels);
}

}  // extern "C"
