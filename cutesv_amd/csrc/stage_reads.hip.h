// stage_reads.hip.h — csv_reads_*: the genotyping reads table in device memory (ReadsTabState in ctx.hip.h, kernels in
// reads.hip.h).  Host code; included by cutesv_hip.hip behind stage_names.hip.h (name_ranks_impl).

// what both appends check first: nothing is launched and nothing changes when one of these fails
static int reads_append_args(csv_ctx* c, const char* what, int chrom, i64 upper)
{
    ReadsTabState& t = c->rt;
    if (t.n_chrom < 0) return fail(c, CSV_E_INVALID, "%s: no csv_reads_reset yet", what);
    if (chrom < 0 || chrom >= t.n_chrom) return fail(c, CSV_E_INVALID, "%s: chromosome %d is outside the %d of csv_reads_reset", what, chrom, t.n_chrom);
    if (chrom < t.last_chrom) return fail(c, CSV_E_INVALID, "%s: chromosome %d comes after rows of chromosome %d", what, chrom, t.last_chrom);
    if (t.n + upper >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "%s: reads table too large (%lld rows)", what, (long long)(t.n + upper));
    return CSV_OK;
}

// room for m more rows behind the committed ones
static int reads_grow(csv_ctx* c, i64 m, ReadsCols* T)
{
    ReadsTabState& t = c->rt;
    TRY(grow_keep(c, t.start, (size_t)(t.n + m) * 4, (size_t)t.n * 4));
    TRY(grow_keep(c, t.end, (size_t)(t.n + m) * 4, (size_t)t.n * 4));
    TRY(grow_keep(c, t.primary, (size_t)(t.n + m), (size_t)t.n));
    TRY(grow_keep(c, t.id, (size_t)(t.n + m) * 4, (size_t)t.n * 4));
    *T = ReadsCols{dp<int>(t.start), dp<int>(t.end), dp<uint8_t>(t.primary), dp<int>(t.id)};
    return CSV_OK;
}

// the call succeeded and m rows lie behind the table: the count moves
static void reads_commit(csv_ctx* c, int chrom, i64 m, i64 max_id)
{
    ReadsTabState& t = c->rt;
    t.n += m; t.last_chrom = chrom;
    t.max_id = std::max(t.max_id, max_id);
    for (int k = chrom + 1; k <= t.n_chrom; k++) t.h_off[(size_t)k] += m;
}

extern "C" {

int csv_reads_reset(csv_ctx* c, int32_t n_chrom)
{
    if (!c) return CSV_E_INVALID;
    if (n_chrom < 0 || n_chrom > (1 << 24)) return fail(c, CSV_E_INVALID, "csv_reads_reset: %d chromosomes", n_chrom);
    ReadsTabState& t = c->rt;
    t.n = 0; t.max_id = -1; t.n_chrom = n_chrom; t.last_chrom = -1;
    t.h_off.assign((size_t)n_chrom + 1, 0);
    return CSV_OK;
}

int csv_reads_rows(const csv_ctx* c, int64_t* n)
{
    if (!c || !n) return CSV_E_INVALID;
    *n = c->rt.n;
    return CSV_OK;
}

int csv_reads_append_decoded(csv_ctx* c, int32_t chrom, int64_t n_records, const uint8_t* keep, int64_t name_base, int64_t* n_appended)
{
    if (!c) return CSV_E_INVALID;
    const char* what = "csv_reads_append_decoded";
    if (n_appended) *n_appended = 0;
    const i64 n = n_records;
    TRY(reads_append_args(c, what, chrom, n_records < 0 ? 0 : n_records));
    if (c->bm.n < 0) return fail(c, CSV_E_INVALID, "%s: the context holds no decoded BAM chunk", what);
    if (n != c->bm.n) return fail(c, CSV_E_INVALID, "%s: n_records is not the record count of the context's last csv_bam_decode", what);
    if (!keep && !c->bm.gates_ok) return fail(c, CSV_E_INVALID, "%s: keep is NULL and the context holds no gates of its last csv_bam_decode (csv_bam_task_gates)", what);
    if (name_base < 0 || name_base + n > (i64)READS_INT_MAX) return fail(c, CSV_E_INVALID, "%s: name ids %lld .. leave 31 bits", what, (long long)name_base);
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    ReadsTabState& t = c->rt;
    // work: the last id and the scan's totals (128 bytes, cleared), per record {keep -> offset}, the tile sums, the caller's keep bytes
    const size_t o_cnt = 128, o_tiles = o_cnt + (((size_t)(n + 1) * 16 + 255) & ~(size_t)255), o_keep = (o_tiles + scan_tile_bytes(n) + 64 + 255) & ~(size_t)255;
    TRY(reserve(c, t.work, o_keep + (keep ? (size_t)n : 0) + 64));
    char* g = (char*)t.work.p;
    int* last_id = (int*)g;
    i64* tot = (i64*)(g + 64);
    int4* cnt = (int4*)(g + o_cnt);
    HIP_TRY(c, hipMemsetAsync(g, 0, 128, st));
    if (keep) HIP_TRY(c, hipMemcpyAsync(g + o_keep, keep, (size_t)n, hipMemcpyHostToDevice, st));
    const uint8_t* flags = keep ? (const uint8_t*)(g + o_keep) : dp<uint8_t>(c->bm.gates);
    const int mask = keep ? 0xff : CSV_GATE_READS;
    TwoPhaseTimer T{c};
    TRY(T.count_begin());
    hipLaunchKernelGGL(k_reads_keep, dim3(div_up(n, 256)), dim3(256), 0, st, flags, mask, n, cnt);
    scan_counts(st, ScanArgs{n, cnt, (i64*)(g + o_tiles), tot});   // the keep flags' exclusive prefix
    TRY(T.count_end());
    i64 m = 0;
    HIP_TRY(c, hipMemcpyAsync(&m, tot, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));                       // (also: the keep bytes have left the caller's array)
    if (m < 0 || m > n) return fail(c, CSV_E_INVALID, "%s: inconsistent row count %lld", what, (long long)m);
    if (m > 0) {
        ReadsCols C{};
        TRY(reads_grow(c, m, &C));
        TRY(T.emit_begin());
        hipLaunchKernelGGL(k_reads_store, dim3(div_up(n, 256)), dim3(256), 0, st, C, t.n, dp<i64>(c->bm.start), dp<i64>(c->bm.end), dp<uint8_t>(c->bm.cls), flags, mask, n,
                           (int)name_base, (const int4*)cnt, m, last_id);
        TRY(T.emit_end());
        int last = -1;
        HIP_TRY(c, hipMemcpyAsync(&last, last_id, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (last < name_base || last >= name_base + n) return fail(c, CSV_E_INVALID, "%s: inconsistent last id %d", what, last);
        reads_commit(c, chrom, m, last);
    }
    TRY(T.elapsed(&t.ms_append));
    if (n_appended) *n_appended = m;
    return CSV_OK;
}

int csv_reads_append(csv_ctx* c, int32_t chrom, int64_t n, const int32_t* start, const int32_t* end, const uint8_t* primary, const int32_t* id)
{
    if (!c) return CSV_E_INVALID;
    const char* what = "csv_reads_append";
    if (n < 0 || (n > 0 && (!start || !end || !primary || !id))) return fail(c, CSV_E_INVALID, "bad reads table append");
    TRY(reads_append_args(c, what, chrom, n));
    i64 max_id = -1;
    for (i64 i = 0; i < n; i++) {
        if (start[i] < 0 || end[i] < start[i] || id[i] < 0)
            return fail(c, CSV_E_INVALID, "%s: row %lld (start %d, end %d, id %d): 0 <= start <= end and id >= 0 are expected", what, (long long)i, start[i], end[i], id[i]);
        max_id = std::max<i64>(max_id, id[i]);
    }
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    ReadsTabState& t = c->rt;
    const size_t o_s = 0, o_e = o_s + (size_t)n * 4, o_i = o_e + (size_t)n * 4, o_p = o_i + (size_t)n * 4;
    TRY(reserve(c, t.work, o_p + (size_t)n + 64));
    ReadsCols C{};
    TRY(reads_grow(c, n, &C));
    char* g = (char*)t.work.p;
    HIP_TRY(c, hipMemcpyAsync(g + o_s, start, (size_t)n * 4, hipMemcpyHostToDevice, st)); HIP_TRY(c, hipMemcpyAsync(g + o_e, end, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(g + o_i, id, (size_t)n * 4, hipMemcpyHostToDevice, st)); HIP_TRY(c, hipMemcpyAsync(g + o_p, primary, (size_t)n, hipMemcpyHostToDevice, st));
    TwoPhaseTimer T{c};
    TRY(T.count_begin());
    hipLaunchKernelGGL(k_reads_put, dim3(div_up(n, 256)), dim3(256), 0, st, C, t.n, (const int*)(g + o_s), (const int*)(g + o_e), (const uint8_t*)(g + o_p), (const int*)(g + o_i), (i64)n);
    TRY(T.count_end());
    HIP_TRY(c, hipStreamSynchronize(st));
    TRY(T.elapsed(&t.ms_append));
    reads_commit(c, chrom, n, max_id);
    return CSV_OK;
}

int csv_reads_get(csv_ctx* c, int64_t first, int64_t n, int32_t* start, int32_t* end, uint8_t* primary, int32_t* id)
{
    if (!c) return CSV_E_INVALID;
    const ReadsTabState& t = c->rt;
    if (first < 0 || n < 0 || first > t.n || n > t.n - first) return fail(c, CSV_E_INVALID, "csv_reads_get: rows [%lld, %lld) of %lld", (long long)first, (long long)(first + n), (long long)t.n);
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (start) HIP_TRY(c, hipMemcpyAsync(start, dp<int>(t.start) + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (end) HIP_TRY(c, hipMemcpyAsync(end, dp<int>(t.end) + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (primary) HIP_TRY(c, hipMemcpyAsync(primary, dp<uint8_t>(t.primary) + first, (size_t)n, hipMemcpyDeviceToHost, st));
    if (id) HIP_TRY(c, hipMemcpyAsync(id, dp<int>(t.id) + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return CSV_OK;
}

int csv_reads_batch_columns(csv_ctx* c, int32_t flags, int32_t n_chrom, int64_t* reads_off, csv_reads_dev* out)
{
    if (!c) return CSV_E_INVALID;
    const char* what = "csv_reads_batch_columns";
    ReadsTabState& t = c->rt;
    if (!reads_off || !out) return fail(c, CSV_E_INVALID, "%s: reads_off and out are needed", what);
    if (t.n_chrom < 0) return fail(c, CSV_E_INVALID, "%s: no csv_reads_reset yet", what);
    if (n_chrom != t.n_chrom) return fail(c, CSV_E_INVALID, "%s: %d chromosomes, the table has %d", what, n_chrom, t.n_chrom);
    if (flags & ~CSV_RD_RANK_FROM_NAMES) return fail(c, CSV_E_INVALID, "%s: unknown flags %d", what, flags);
    const bool by_rank = (flags & CSV_RD_RANK_FROM_NAMES) != 0;
    if (by_rank && t.max_id >= c->nm.n) return fail(c, CSV_E_INVALID, "%s: the table holds name id %lld, the name pool %lld names", what, (long long)t.max_id, (long long)c->nm.n);
    t.ms_columns = 0;
    const int* r_id = dp<int>(t.id);
    if (by_rank && t.n > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        TRY(name_ranks_impl(c));                                // (nothing to do while the ranks are fresh)
        TRY(reserve(c, t.rid, (size_t)t.n * 4));
        hipStream_t st = c->stream;
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(k_reads_rank, dim3(div_up(t.n, 256)), dim3(256), 0, st, dp<int>(t.id), dp<int>(c->nm.rank), dp<int>(t.rid), t.n);
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(st));                   // (the engine reads the columns from streams of its own)
        HIP_TRY(c, hipEventElapsedTime(&t.ms_columns, c->ev[0], c->ev[1]));
        r_id = dp<int>(t.rid);
    }
    for (int k = 0; k <= n_chrom; k++) reads_off[k] = t.h_off[(size_t)k];
    out->n_reads = t.n;
    out->r_start = t.n ? dp<int>(t.start) : nullptr; out->r_end = t.n ? dp<int>(t.end) : nullptr;
    out->r_primary = t.n ? dp<uint8_t>(t.primary) : nullptr; out->r_id = t.n ? r_id : nullptr;
    return CSV_OK;
}

int csv_reads_timing(const csv_ctx* c, float* ms_append, float* ms_columns)
{
    if (!c) return CSV_E_INVALID;
    if (ms_append) *ms_append = c->rt.ms_append;
    if (ms_columns) *ms_columns = c->rt.ms_columns;
    return CSV_OK;
}

int csv_reads_struct_size(int which) { return which == 0 ? (int)sizeof(csv_reads_dev) : -1; }

}  // extern "C"
