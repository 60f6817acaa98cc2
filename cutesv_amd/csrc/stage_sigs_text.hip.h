// stage_sigs_text.hip.h — csv_pool_sigs_text: rows of the last kept pool rebuild as the text lines of cuteSV's <TYPE>.sigs files, made on
// the device from the sorted columns and the pools they number (kernels at the end of vcf_strings.hip.h; the readiness rule and the scratch are those of
// the VCF strings, VcfStrState in ctx.hip.h).  Host code; included by cutesv_hip.hip behind stage_vcf_strings.hip.h.

extern "C" {

int csv_pool_sigs_text(csv_ctx* c, int64_t row_begin, int64_t row_end, const char* chrom_names, const int64_t* chrom_off, int32_t n_chrom, const char* strand0,
                       const char* strand1, char* out, int64_t cap, int64_t* need, float* ms_kernels)
{
    if (!c) return CSV_E_INVALID;
    if (!need || cap < 0 || (cap > 0 && !out) || n_chrom < 1 || n_chrom > (1 << 24) || !chrom_off || !strand0 || !strand1) return fail(c, CSV_E_INVALID, "bad sigs text");
    *need = 0;
    if (ms_kernels) *ms_kernels = 0;
    TRY(vs_ready(c, "csv_pool_sigs_text"));
    if (!c->vs.by_name || !c->nm.fresh) return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: the kept rebuild's read ids are not ranks of the name pool (CSV_RB_RANK_FROM_NAMES)");
    if (row_begin < 0 || row_end < row_begin || row_end > c->vs.n_out)
        return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: rows [%lld, %lld) lie outside the %lld rows of the rebuild", (long long)row_begin, (long long)row_end, (long long)c->vs.n_out);
    // the caller's tables are checked before anything is launched
    if (chrom_off[0] != 0) return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: chrom_off must start at 0");
    for (int k = 0; k < n_chrom; k++)
        if (chrom_off[k + 1] < chrom_off[k]) return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: chrom_off decreases at chromosome %d", k);
    const i64 name_bytes = chrom_off[n_chrom];
    if (name_bytes >= (1ll << 30) || (name_bytes > 0 && !chrom_names)) return fail(c, CSV_E_INVALID, "bad sigs text");
    StTables T{};
    const char* strands[2] = {strand0, strand1};
    for (int k = 0; k < 2; k++) {
        const size_t l = strlen(strands[k]);
        if (l > ST_STRAND_MAX) return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: a strand string is longer than %d bytes", ST_STRAND_MAX);
        memcpy(T.strand[k], strands[k], l);
        T.strand_len[k] = (int)l;
    }
    const i64 n = row_end - row_begin;
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    SeqState& s = c->seq;
    if (s.off.p) TRY(seq_sync(c, c->pool.n));
    VcfStrState& v = c->vs;
    hipStream_t st = c->stream;
    // vs.work: chromosome offsets (int), their names, then the lengths, the scan's tile sums and its totals
    std::vector<int> coff((size_t)n_chrom + 1);
    for (int k = 0; k <= n_chrom; k++) coff[(size_t)k] = (int)chrom_off[k];
    const size_t o_names = (size_t)(n_chrom + 1) * 4, o_cnt = (o_names + (size_t)name_bytes + 255) & ~(size_t)255,
                 o_tiles = o_cnt + (((size_t)(n + 1) * 16 + 255) & ~(size_t)255), o_tot = o_tiles + ((scan_tile_bytes(n) + 255) & ~(size_t)255);
    TRY(reserve(c, v.work, o_tot + 64));
    char* g = (char*)v.work.p;
    int4* cnt = (int4*)(g + o_cnt);
    i64* tot = (i64*)(g + o_tot);
    int* err = (int*)(tot + 4);
    HIP_TRY(c, hipMemcpyAsync(g, coff.data(), o_names, hipMemcpyHostToDevice, st));
    if (name_bytes > 0) HIP_TRY(c, hipMemcpyAsync(g + o_names, chrom_names, (size_t)name_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(tot, 0, 40, st));
    T.chrom = (const uint8_t*)(g + o_names); T.chrom_off = (const int*)g; T.n_chrom = n_chrom;
    T.seq_blob = dp<uint8_t>(s.blob); T.seq_off = s.off.p ? dp<i64>(s.off) : nullptr;
    const StRows R{dp<int>(c->rb.oseg), dp<i64>(c->rb.oa), dp<i64>(c->rb.ob), dp<int>(c->rb.orid), dp<int>(c->rb.oaux), dp<int>(c->rb.osrc)};
    const VsNames N{dp<uint8_t>(c->nm.blob), dp<i64>(c->nm.off), dp<int>(c->nm.first), c->nm.distinct};
    TwoPhaseTimer tm{c};
    TRY(tm.count_begin());
    hipLaunchKernelGGL(k_sigs_plan, dim3(vs_grid_threads(n)), dim3(256), 0, st, R, N, T, (i64)row_begin, n, cnt, err);
    scan_counts(st, ScanArgs{n, cnt, (i64*)(g + o_tiles), tot});   // the lengths' exclusive prefix
    TRY(tm.count_end());
    i64 got[5] = {0, 0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(got, tot, 40, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));                          // (coff was an upload's source)
    const int e = (int)(got[4] & 0xffffffffll);
    if (e)
        return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: %s",
                    (e & ST_ERR_SEG)      ? "a row's segment lies outside 5 * n_chrom"
                    : (e & ST_ERR_COORD)  ? "a position or length is negative or at least 2^42"
                    : (e & ST_ERR_RANK)   ? "a row's read id is no rank of the name pool"
                    : (e & ST_ERR_NO_SEQ) ? "an INS row has no sequence in the sequence pool"
                    : (e & ST_ERR_STRAND) ? "an INV row's strand code is above 1"
                                          : "a TRA row's type code is above 3 or its mate chromosome lies outside the table");
    if (got[0] < 0 || got[0] >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "csv_pool_sigs_text: %lld bytes in one call: ask for fewer rows", (long long)got[0]);
    *need = got[0];
    if (got[0] > cap) return fail(c, CSV_E_CAPACITY, "out: %lld bytes are needed", (long long)got[0]);
    TRY(reserve(c, v.out, (size_t)got[0] + 8));
    TRY(tm.emit_begin());
    hipLaunchKernelGGL(k_sigs_write, dim3(vs_grid_waves(n)), dim3(256), 0, st, R, N, T, (i64)row_begin, n, cnt, dp<uint8_t>(v.out));
    TRY(tm.emit_end());
    HIP_TRY(c, hipMemcpyAsync(out, v.out.p, (size_t)got[0], hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (ms_kernels) TRY(tm.elapsed(ms_kernels));
    return CSV_OK;
}

}  // extern "C"
