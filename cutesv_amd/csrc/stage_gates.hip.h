// stage_gates.hip.h — csv_bam_task_gates: the gates of an extraction task as a byte column beside the decoded records (BamState
// in ctx.hip.h; gates.hip.h).  Host code; included by cutesv_hip.hip.
extern "C" {

int csv_bam_task_gates(csv_ctx* c, int64_t n_records, int64_t task_start, int32_t min_read_len, int32_t min_mapq, int32_t flags, int64_t n_regions,
                       const int64_t* region_beg, const int64_t* region_end, uint8_t* bits, float* ms_device)
{
    if (!c) return CSV_E_INVALID;
    const char* what = "csv_bam_task_gates";
    if (ms_device) *ms_device = 0;
    const i64 n = n_records, nr = n_regions;
    const bool bed = (flags & CSV_GT_BED) != 0;
    // everything is checked before anything is launched: a refused call leaves the context - and the gates it holds - as they were
    if (c->bm.n < 0) return fail(c, CSV_E_INVALID, "%s: the context holds no decoded BAM chunk", what);
    if (n != c->bm.n) return fail(c, CSV_E_INVALID, "%s: n_records is not the record count of the context's last csv_bam_decode", what);
    if (flags & ~CSV_GT_BED) return fail(c, CSV_E_INVALID, "%s: unknown flags %d", what, flags);
    if (nr < 0) return fail(c, CSV_E_INVALID, "%s: %lld regions", what, (long long)nr);
    if (!bed && (nr > 0 || region_beg || region_end)) return fail(c, CSV_E_INVALID, "%s: regions are given without CSV_GT_BED", what);
    if (bed && nr > 0 && (!region_beg || !region_end)) return fail(c, CSV_E_INVALID, "%s: CSV_GT_BED with %lld regions and no array", what, (long long)nr);
    if (nr >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "%s: too many regions (%lld)", what, (long long)nr);
    for (i64 k = 1; k < nr; k++)                              // the kernel searches region_beg by halving
        if (region_beg[k] < region_beg[k - 1]) return fail(c, CSV_E_INVALID, "%s: region_beg decreases at region %lld", what, (long long)k);
    if (n == 0) { c->bm.gates_ok = true; return CSV_OK; }
    HIP_TRY(c, hipSetDevice(c->device));
    c->bm.gates_ok = false;
    hipStream_t st = c->stream;
    TRY(reserve(c, c->bm.gates, (size_t)n));
    if (nr > 0) {
        HIP_TRY(c, hipStreamSynchronize(st));                   // (an earlier call that failed half way may still be copying out of gtab_h)
        std::vector<i64>& tab = c->bm.gtab_h;                   // region_beg, then the running maximum of region_end
        tab.resize((size_t)nr * 2);
        TRY(reserve(c, c->bm.gtab, (size_t)nr * 16));
        i64 mx = region_end[0];
        for (i64 k = 0; k < nr; k++) {
            tab[(size_t)k] = region_beg[k];
            mx = region_end[k] > mx ? region_end[k] : mx;
            tab[(size_t)(nr + k)] = mx;
        }
        TRY(h2d(c, c->bm.gtab, tab.data(), nr * 16));
    }
    GateArgs A{};
    A.n = n; A.ref_start = dp<i64>(c->bm.start); A.ref_end = dp<i64>(c->bm.end); A.mapq = dp<int>(c->bm.mapq); A.qlen = dp<int>(c->bm.qlen);
    A.cls = dp<uint8_t>(c->bm.cls); A.sa_off = dp<i64>(c->bm.saoff);
    A.task_start = task_start; A.min_read_len = min_read_len; A.min_mapq = min_mapq; A.bed = bed ? 1 : 0;
    A.n_regions = nr; A.beg = nr > 0 ? dp<i64>(c->bm.gtab) : nullptr; A.pmax_end = nr > 0 ? dp<i64>(c->bm.gtab) + nr : nullptr;
    A.bits = dp<uint8_t>(c->bm.gates);
    const int grid = div_up(n, 256) < 4096 ? div_up(n, 256) : 4096;
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_task_gates, dim3(grid), dim3(256), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    TRY(d2h(c, bits, c->bm.gates, n, false));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (ms_device) HIP_TRY(c, hipEventElapsedTime(ms_device, c->ev[0], c->ev[1]));
    c->bm.gates_ok = true;
    return CSV_OK;
}

}  // extern "C"
