// stage_vcf_emit.hip.h — csv_vcf_emit_device: the VCF records of a batch's calls written on the device (k_vcf_plan / k_vcf_len / k_vcf_write at
// the end of vcf_strings.hip.h over vcf_core.h), the text kept in device memory on request, and the two entries that
// read a kept text: csv_vcf_text_info / csv_vcf_text_fetch.  (csv_bgzf_deflate_text, which compresses it, stands with its sibling in
// stage_deflate.hip.h.)  The device buffers are VcfEmitState's own (ctx.hip.h).  Host code; included by cutesv_hip.hip behind
// stage_vcf_strings.hip.h and stage_deflate.hip.h.

#include "soa_access.h"

// host bytes -> a slot of `b` at offset `at` (8-aligned by the caller); nothing to do for zero bytes
static int ve_put(csv_ctx* c, const Buf& b, size_t at, const void* src, i64 bytes)
{
    if (bytes > 0) HIP_TRY(c, hipMemcpyAsync((char*)b.p + at, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    return CSV_OK;
}

extern "C" {

int csv_vcf_emit_device(csv_ctx* c, const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, int64_t n_pick, const int64_t* pick, const int64_t* clip, const char* prefix,
                        int64_t prefix_bytes, int32_t flags, char* out, int64_t cap, int64_t* n_written, int64_t* svid, int64_t* rows, int64_t rows_cap, int64_t* n_rows,
                        int32_t* name_chrom, int32_t* n_names, double* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (ms_kernels) *ms_kernels = 0;
    if (!in || !in->res || !ref_off || !n_written || !svid || !n_rows || cap < 0 || rows_cap < 0 || prefix_bytes < 0 || (prefix_bytes > 0 && !prefix) || (cap > 0 && !out) ||
        (rows_cap > 0 && !rows) || (flags & ~(CSV_VCF_KEEP_TEXT | CSV_VCF_ALT_FROM_POOL | CSV_VCF_RNAMES_FROM_POOL)) || (rows && in->n_chrom > 0 && (!name_chrom || !n_names)))
        return fail(c, CSV_E_INVALID, "bad vcf emit");
    const bool alt_pool = (flags & CSV_VCF_ALT_FROM_POOL) && !in->ignore_sequence, rn_pool = (flags & CSV_VCF_RNAMES_FROM_POOL) && in->report_readid;
    if ((flags & CSV_VCF_ALT_FROM_POOL) && (n_pick < 0 || (n_pick > 0 && (!pick || !clip)))) return fail(c, CSV_E_INVALID, "bad vcf emit");
    const csv_batch_out& R = *in->res;
    const i64 nc = R.n_calls;
    // everything the kernels trust is judged on the host before anything is launched: the columns are host arrays
    csv_vcf_in in2 = *in;
    std::vector<int64_t> alt_off, rn_off;
    static const char kOnDevice = 0;                              // (a blob that lies on the device: prepare reads its offsets, never its bytes)
    if (alt_pool) { in2.ins_alt = nullptr; in2.ins_alt_off = nullptr; }
    if (rn_pool) { in2.rnames = nullptr; in2.rnames_off = nullptr; }
    VcfHost H;
    if (vcf_host_prepare(&in2, ref_blob, ref_off, H) != CSV_OK)
        return fail(c, CSV_E_INVALID, "csv_vcf_emit_device: the calls do not fit their tables (a segment, chromosome, strand or mate chromosome out of range, a gl_idx without a "
                                      "table row, a range outside its contig, REF bytes that are not as many as the range, or DV and DR that give no allele frequency)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    VcfEmitState& e = c->ve;
    // the strings of a kept rebuild: the existing plan, offset and copy kernels, their blobs left where k_vcf_write reads them
    if (alt_pool) {
        i64 n_ins = 0;
        for (i64 k = 0; k < nc; k++) n_ins += in->seg[R.call_seg[k]].svtype == CSV_INS;
        if (n_pick != n_ins) return fail(c, CSV_E_INVALID, "csv_vcf_emit_device: %lld picks for %lld INS calls", (long long)n_pick, (long long)n_ins);
        std::vector<int64_t> off((size_t)n_pick + 1, 0);
        TRY(alt_gather_run(c, n_pick, pick, clip, 0, nullptr, 0, off.data(), &e.alt));
        alt_off.assign((size_t)nc + 1, 0);
        for (i64 k = 0, j = 0; k < nc; k++) {
            const bool ins = in->seg[R.call_seg[k]].svtype == CSV_INS;
            alt_off[(size_t)k + 1] = alt_off[(size_t)k] + (ins ? off[(size_t)j + 1] - off[(size_t)j] : 0);
            j += ins;
        }
        in2.ins_alt = &kOnDevice; in2.ins_alt_off = alt_off.data();
    }
    if (rn_pool) {
        if (!csv_soa::has_support_list(R)) return fail(c, CSV_E_INVALID, "csv_vcf_emit_device: CSV_VCF_RNAMES_FROM_POOL needs the result's support lists");
        rn_off.assign((size_t)nc + 1, 0);
        TRY(support_join_run(c, nc, R.support_off, R.support_sig, R.support_sig ? nullptr : R.support_sig32, nullptr, 0, rn_off.data(), &e.rn));
        in2.rnames = &kOnDevice; in2.rnames_off = rn_off.data();
    }
    if ((alt_pool || rn_pool) && vcf_host_prepare(&in2, ref_blob, ref_off, H) != CSV_OK) return fail(c, CSV_E_INVALID, "csv_vcf_emit_device: the gathered strings do not fit the calls");
    const i64 n = (i64)H.order.size();
    if (H.ref_bytes + H.alt_bytes + H.rn_bytes + prefix_bytes >= (1ll << 31) - 4096)
        return fail(c, CSV_E_INVALID, "csv_vcf_emit_device: %lld bytes in one call: split the batch", (long long)(H.ref_bytes + H.alt_bytes + H.rn_bytes + prefix_bytes));
    e.kept = false; e.gen++; e.text_bytes = 0;                     // the next emit drops a kept text
    *n_rows = 0;
    if (n_names) *n_names = 0;
    // blobs: REF | ALT | RNAMES (the host's; a pooled one lies in its own buffer)
    const i64 alt_up = alt_pool ? 0 : H.alt_bytes, rn_up = rn_pool ? 0 : H.rn_bytes;
    const size_t b_alt = ((size_t)H.ref_bytes + 7) & ~(size_t)7, b_rn = b_alt + (((size_t)alt_up + 7) & ~(size_t)7), b_end = b_rn + (((size_t)rn_up + 7) & ~(size_t)7);
    TRY(reserve(c, e.blobs, b_end + 8));
    TRY(ve_put(c, e.blobs, 0, ref_blob, H.ref_bytes));
    TRY(ve_put(c, e.blobs, b_alt, in2.ins_alt, alt_up));
    TRY(ve_put(c, e.blobs, b_rn, in2.rnames, rn_up));
    // work: the view's tables | order | three count columns | the scan's tile sums | 3 x 3 totals
    const size_t pack = (H.pack.size() + 255) & ~(size_t)255, o_order = pack, o_a = (o_order + (size_t)n * 8 + 255) & ~(size_t)255, col = ((size_t)(n + 1) * 16 + 255) & ~(size_t)255,
                 o_b = o_a + col, o_c = o_b + col, o_tiles = o_c + col, o_tot = o_tiles + ((scan_tile_bytes(n > 0 ? n : 1) + 255) & ~(size_t)255);
    TRY(reserve(c, e.work, o_tot + 128));
    char* g = (char*)e.work.p;
    TRY(ve_put(c, e.work, 0, H.pack.data(), (i64)H.pack.size()));
    TRY(ve_put(c, e.work, o_order, H.order.data(), n * 8));
    int4 *cnt_a = (int4*)(g + o_a), *cnt_b = (int4*)(g + o_b), *cnt_c = (int4*)(g + o_c);
    i64* tot = (i64*)(g + o_tot);                                 // [0..2] INS DEL BND, [4..6] DUP INV emitted, [8] bytes
    HIP_TRY(c, hipMemsetAsync(tot, 0, 96, st));
    uint8_t* blobs = dp<uint8_t>(e.blobs);
    VeArgs A{};
    A.V = vcf_view_moved(H, g, blobs, alt_pool ? dp<uint8_t>(e.alt) : blobs + b_alt, rn_pool ? dp<uint8_t>(e.rn) : blobs + b_rn);
    A.order = (const i64*)(g + o_order); A.n = n;
    A.sv_ins = svid[0]; A.sv_del = svid[1]; A.sv_bnd = svid[2]; A.sv_dup = svid[3]; A.sv_inv = svid[4];
    A.prefix = prefix_bytes;
    TwoPhaseTimer tm{c};
    TRY(tm.count_begin());
    if (n > 0) {
        hipLaunchKernelGGL(k_vcf_plan, dim3(vs_grid_threads(n)), dim3(256), 0, st, A, cnt_a, cnt_b);
        scan_counts(st, ScanArgs{n, cnt_a, (i64*)(g + o_tiles), tot});
        scan_counts(st, ScanArgs{n, cnt_b, (i64*)(g + o_tiles), tot + 4});
        hipLaunchKernelGGL(k_vcf_len, dim3(vs_grid_threads(n)), dim3(256), 0, st, A, (const int4*)cnt_a, (const int4*)cnt_b, cnt_c);
        scan_counts(st, ScanArgs{n, cnt_c, (i64*)(g + o_tiles), tot + 8});
    }
    TRY(tm.count_end());
    i64 got[12] = {0};
    HIP_TRY(c, hipMemcpyAsync(got, tot, 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));                          // (H's vectors were the uploads' sources)
    const i64 n_rec = got[6], need = prefix_bytes + got[8];
    if (got[8] < 0 || need >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "csv_vcf_emit_device: %lld bytes in one call: split the batch", (long long)need);
    *n_written = need;
    *n_rows = n_rec;
    const bool keep = (flags & CSV_VCF_KEEP_TEXT) != 0;
    if ((!keep || out) && (!out || need > cap)) return fail(c, CSV_E_CAPACITY, "out: %lld bytes are needed", (long long)need);
    if (rows && n_rec > rows_cap) return fail(c, CSV_E_CAPACITY, "rows: %lld rows are needed", (long long)n_rec);
    TRY(reserve(c, e.text, (size_t)need + 64));
    TRY(reserve(c, e.rows, (size_t)n_rec * 32 + 64));
    TRY(ve_put(c, e.text, 0, prefix, prefix_bytes));
    TRY(tm.emit_begin());
    if (n_rec > 0) hipLaunchKernelGGL(k_vcf_write, dim3(vs_grid_waves(n)), dim3(256), 0, st, A, (const int4*)cnt_a, (const int4*)cnt_b, (const int4*)cnt_c, dp<uint8_t>(e.text), dp<i64>(e.rows));
    TRY(tm.emit_end());
    if (out && need > 0) HIP_TRY(c, hipMemcpyAsync(out, e.text.p, (size_t)need, hipMemcpyDeviceToHost, st));
    if (rows && n_rec > 0) HIP_TRY(c, hipMemcpyAsync(rows, e.rows.p, (size_t)n_rec * 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (rows) {                                                    // chromosome -> name index, in order of first appearance
        std::vector<int32_t> name_of((size_t)in->n_chrom, -1);
        int32_t nn = 0;
        for (i64 r = 0; r < n_rec; r++) {
            int32_t& k = name_of[(size_t)rows[4 * r]];
            if (k < 0) { k = nn; name_chrom[nn++] = (int32_t)rows[4 * r]; }
            rows[4 * r] = k;
        }
        *n_names = nn;
    }
    if (ms_kernels) { float ms = 0; TRY(tm.elapsed(&ms)); *ms_kernels = ms; }
    for (int t = 0; t < 3; t++) svid[t] += got[t];
    svid[3] += got[4]; svid[4] += got[5];
    if (keep) { e.kept = true; e.text_bytes = need; }
    return CSV_OK;
}

// the kept text: *gen <- the number of emits this context has seen (a handle made after emit k is good while gen == k), *bytes <- its size,
// 0 when nothing is kept
int csv_vcf_text_info(csv_ctx* c, int64_t* gen, int64_t* bytes)
{
    if (!c) return CSV_E_INVALID;
    if (gen) *gen = (int64_t)c->ve.gen;
    if (bytes) *bytes = c->ve.kept ? c->ve.text_bytes : 0;
    return CSV_OK;
}

int csv_vcf_text_fetch(csv_ctx* c, char* out, int64_t cap, int64_t* need)
{
    if (!c) return CSV_E_INVALID;
    if (!need || cap < 0 || (cap > 0 && !out)) return fail(c, CSV_E_INVALID, "bad vcf text fetch");
    if (!c->ve.kept) return fail(c, CSV_E_INVALID, "csv_vcf_text_fetch: the context keeps no VCF text (csv_vcf_emit_device with CSV_VCF_KEEP_TEXT)");
    *need = c->ve.text_bytes;
    if (c->ve.text_bytes > cap) return fail(c, CSV_E_CAPACITY, "out: %lld bytes are needed", (long long)c->ve.text_bytes);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->ve.text_bytes > 0) HIP_TRY(c, hipMemcpyAsync(out, c->ve.text.p, (size_t)c->ve.text_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CSV_OK;
}

}  // extern "C"
