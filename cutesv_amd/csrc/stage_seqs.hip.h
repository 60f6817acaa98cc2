// stage_seqs.hip.h — the INS sequence pool (SeqState in ctx.hip.h, kernels in seqs.hip.h): csv_seq_reads_upload, the attach step
// of the entries that append INS rows (CSV_CG_SEQ_TO_POOL), csv_seq_pool_*, and the device's answer to the rebuild's INS tie
// groups (CSV_RB_TIES_FROM_SEQS).  Host code; included by cutesv_hip.hip.
extern "C" {

// the row arrays hold a value for every pool row below `upto`: rows appended without a sequence get "none"
static int seq_sync(csv_ctx* c, i64 upto)
{
    SeqState& s = c->seq;
    TRY(seq_rows_reserve(c, std::max<i64>(std::max(upto, c->pool.cap), 1)));
    if (upto > s.rows) {
        HIP_TRY(c, hipMemsetAsync(dp<i64>(s.off) + s.rows, 0xff, (size_t)(upto - s.rows) * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(dp<uint8_t>(s.half) + s.rows, 0, (size_t)(upto - s.rows), c->stream));
        s.rows = upto;
    }
    return CSV_OK;
}

static const char* seq_why(int err)
{
    return (err & SEQ_ERR_NO_READ) ? "a row's read has no uploaded sequence (csv_seq_reads_upload; the `want` column)"
         : (err & SEQ_ERR_NEGATIVE) ? "a CIGAR piece has a negative offset or length"
         : (err & SEQ_ERR_TAKEN) ? "a row has a sequence already"
         : "the length of a row's bases is not its aux (query_len must be the uploaded l_seq)";
}

// csv_seq_reads_upload; with dev_bytes (csv_seq_reads_framed, stage_frame.hip.h) the n_bytes bytes lie in device memory and the wanted
// reads are packed there (k_frame_gather): what crosses the link is the offset and length tables alone
static int seq_reads_upload_impl(csv_ctx* c, int64_t n, const uint8_t* bytes, const uint8_t* dev_bytes, int64_t n_bytes, const int64_t* off, const int32_t* l_seq, const uint8_t* want)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || n_bytes < 0 || (n > 0 && (!off || !l_seq)) || (n_bytes > 0 && !bytes && !dev_bytes)) return fail(c, CSV_E_INVALID, "bad read sequence upload");
    if (n >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "too many reads (%lld): split the batch", (long long)n);
    // every range is checked before the state changes or anything is launched
    i64 total = 0, n_want = 0;
    for (i64 i = 0; i < n; i++) {
        const i64 nb = ((i64)l_seq[i] + 1) / 2;
        if (l_seq[i] < 0 || off[i] < 0 || off[i] > n_bytes || nb > n_bytes - off[i])
            return fail(c, CSV_E_INVALID, "read %lld: its %lld packed bytes at %lld leave the %lld bytes given", (long long)i, (long long)nb, (long long)off[i], (long long)n_bytes);
        if (!want || want[i]) { total += nb; n_want++; }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    SeqState& s = c->seq;
    // the wanted reads are packed back to back first (CSV_SEQ_OPT_WHOLE_IMAGE, a measurement aid: the image goes as it is)
    const bool whole = s.whole && !dev_bytes;
    std::vector<uint8_t> img;
    std::vector<int> nbs(dev_bytes ? (size_t)n : 0);
    std::vector<i64> offs((size_t)n);
    std::vector<int> lens((size_t)n);
    if (!whole && !dev_bytes) img.resize((size_t)total);
    i64 at = 0;
    for (i64 i = 0; i < n; i++) {
        const bool w = !want || want[i];
        const i64 nb = w ? ((i64)l_seq[i] + 1) / 2 : 0;
        lens[(size_t)i] = w ? l_seq[i] : -1;
        offs[(size_t)i] = whole ? off[i] : at;
        if (!whole && nb && !dev_bytes) memcpy(img.data() + at, bytes + off[i], (size_t)nb);
        if (dev_bytes) nbs[(size_t)i] = (int)nb;
        at += nb;
    }
    const i64 sent = whole ? n_bytes : total;
    s.n_reads = -1; s.n_qrev = -1;
    TRY(reserve(c, s.rbytes, (size_t)sent + 8)); TRY(reserve(c, s.roff, (size_t)n * 8 + 8)); TRY(reserve(c, s.rlen, (size_t)n * 4 + 8));
    if (!dev_bytes) TRY(h2d(c, s.rbytes, whole ? bytes : img.data(), sent));
    TRY(h2d(c, s.roff, offs.data(), n * 8)); TRY(h2d(c, s.rlen, lens.data(), n * 4));
    if (dev_bytes && total) TRY(frame_gather(c, n, dev_bytes, off, nbs.data(), dp<uint8_t>(s.rbytes), dp<i64>(s.roff)));
    HIP_TRY(c, hipStreamSynchronize(c->stream));             // (the vectors are the copies' sources)
    s.n_reads = n;
    s.info.reads_uploaded = n_want; s.info.bytes_uploaded = (dev_bytes ? 0 : sent) + n * 12; s.info.packed = whole ? 0 : 1;
    s.info.ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return CSV_OK;
}

int csv_seq_reads_upload(csv_ctx* c, int64_t n, const uint8_t* bytes, int64_t n_bytes, const int64_t* off, const int32_t* l_seq, const uint8_t* want)
{
    return seq_reads_upload_impl(c, n, bytes, nullptr, n_bytes, off, l_seq, want);
}

int csv_seq_option(csv_ctx* c, int which, int value)
{
    if (!c) return CSV_E_INVALID;
    if (which != CSV_SEQ_OPT_WHOLE_IMAGE) return fail(c, CSV_E_INVALID, "csv_seq_option: unknown option %d", which);
    c->seq.whole = value != 0;
    return CSV_OK;
}

int csv_seq_query_reverse(csv_ctx* c, int64_t n, const uint8_t* reverse)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || (n > 0 && !reverse)) return fail(c, CSV_E_INVALID, "bad query_reverse column");
    if (n != c->seq.n_reads) return fail(c, CSV_E_INVALID, "query_reverse: %lld entries for the %lld reads of the last csv_seq_reads_upload", (long long)n, (long long)c->seq.n_reads);
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(reserve(c, c->seq.qrev, (size_t)n + 8));
    TRY(h2d(c, c->seq.qrev, reverse, n));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->seq.n_qrev = n;
    return CSV_OK;
}

}  // extern "C"

// The sequence step of an entry that appends `rows` rows at pool row c->pool.n (before it adds them to the count), the first
// n_plan of which may be INS rows: plan(cnt, err) launches the length kernel, gather(cnt, pool, blob_base) the copy.  On
// CSV_E_INVALID nothing of the sequence pool has changed and the entry must not count the rows.
template <class PlanFn, class GatherFn> static int seq_attach(csv_ctx* c, i64 rows, i64 n_plan, PlanFn plan, GatherFn gather)
{
    SeqState& s = c->seq;
    hipStream_t st = c->stream;
    const size_t o_tiles = ((size_t)(n_plan + 1) * 16 + 255) & ~(size_t)255, o_tot = o_tiles + scan_tile_bytes(n_plan > 0 ? n_plan : 1) + 8;
    TRY(reserve(c, s.plan, o_tot + 64));
    int4* cnt = (int4*)s.plan.p;
    i64* tot = (i64*)((char*)s.plan.p + ((o_tot + 7) & ~(size_t)7));
    int* err = (int*)(tot + 4);
    HIP_TRY(c, hipMemsetAsync(tot, 0, 40, st));
    HIP_TRY(c, hipEventRecord(c->ev[6], st));
    i64 got[5] = {0, 0, 0, 0, 0};
    if (n_plan > 0) {
        plan(cnt, err);
        scan_counts(st, ScanArgs{n_plan, cnt, (i64*)((char*)s.plan.p + o_tiles), tot});   // the lengths' exclusive prefix
    }
    HIP_TRY(c, hipEventRecord(c->ev[7], st));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(got, tot, 40, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const int e = (int)(got[4] & 0xffffffffll);
    if (e) return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL: %s", seq_why(e));
    const i64 total = got[0], n_with = got[1];
    if (total < 0 || total >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL: %lld bases in one call: split the batch", (long long)total);
    TRY(grow_keep(c, s.blob, (size_t)(s.bytes + total) + 8, (size_t)s.bytes));
    const i64 base = c->pool.n;
    TRY(seq_sync(c, base + rows));                              // (every new row: none, until the gather says otherwise)
    s.rows = base;                                              // ... and they count only once the gather went through
    HIP_TRY(c, hipEventRecord(c->ev[8], st));
    if (n_plan > 0) gather(cnt, SeqPool{dp<uint8_t>(s.blob), dp<i64>(s.off), dp<uint8_t>(s.half)}, s.bytes);
    HIP_TRY(c, hipEventRecord(c->ev[9], st));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms1 = 0, ms2 = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms1, c->ev[6], c->ev[7])); HIP_TRY(c, hipEventElapsedTime(&ms2, c->ev[8], c->ev[9]));
    s.info.ms_gather = ms1 + ms2; s.info.rows_gathered = n_with; s.info.bytes_gathered = total;
    s.rows = base + rows; s.bytes += total; s.n_with += n_with;
    return CSV_OK;
}

extern "C" {

int csv_seq_pool_rows(const csv_ctx* c, int64_t* n_with_seq, int64_t* n_bytes)
{
    if (!c || !n_with_seq || !n_bytes) return CSV_E_INVALID;
    *n_with_seq = c->seq.n_with; *n_bytes = c->seq.bytes;
    return CSV_OK;
}

int csv_seq_info_get(const csv_ctx* c, csv_seq_info* out)
{
    if (!c || !out) return CSV_E_INVALID;
    *out = c->seq.info;
    out->device_bytes = const_cast<csv_ctx*>(c)->seq.device_bytes();
    return CSV_OK;
}

// the requested pool rows on the device, after the range check every entry below shares
static int seq_rows_in(csv_ctx* c, const char* what, i64 n, const int32_t* pool_row, Buf& buf, size_t extra, int** d_rows)
{
    for (i64 k = 0; k < n; k++)
        if (pool_row[k] < 0 || pool_row[k] >= c->pool.n) return fail(c, CSV_E_INVALID, "%s: pool_row[%lld] = %d is outside the %lld rows of the pool", what, (long long)k, pool_row[k], (long long)c->pool.n);
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(seq_sync(c, c->pool.n));
    TRY(reserve(c, buf, (size_t)n * 4 + 64 + extra));
    *d_rows = (int*)buf.p;
    HIP_TRY(c, hipMemcpyAsync(buf.p, pool_row, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    return CSV_OK;
}

int csv_seq_pool_put(csv_ctx* c, int64_t n, const int32_t* pool_row, const uint8_t* bytes, int64_t n_bytes, const int64_t* off, const int32_t* len, const uint8_t* half)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || n_bytes < 0 || (n > 0 && (!pool_row || !off || !len)) || (n_bytes > 0 && !bytes)) return fail(c, CSV_E_INVALID, "bad sequence pool put");
    if (n == 0) return CSV_OK;
    i64 total = 0;
    for (i64 k = 0; k < n; k++) {
        if (len[k] < 0 || off[k] < 0 || off[k] > n_bytes || (i64)len[k] > n_bytes - off[k])
            return fail(c, CSV_E_INVALID, "sequence %lld: bytes [%lld, %lld) leave the %lld bytes given", (long long)k, (long long)off[k], (long long)off[k] + len[k], (long long)n_bytes);
        total += len[k];
    }
    std::vector<int> sorted(pool_row, pool_row + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(c, CSV_E_INVALID, "csv_seq_pool_put: a pool row is named twice");
    SeqState& s = c->seq;
    // one buffer: rows, lengths, blob offsets (8-byte aligned), x.5 flags, the error word
    const size_t o_len = (size_t)n * 4, o_at = ((o_len + (size_t)n * 4) + 7) & ~(size_t)7, o_half = o_at + (size_t)n * 8, o_err = (o_half + (size_t)n + 7) & ~(size_t)7;
    int* d_rows = nullptr;
    TRY(seq_rows_in(c, "csv_seq_pool_put", n, pool_row, s.get, o_err + 8, &d_rows));
    hipStream_t st = c->stream;
    char* g = (char*)s.get.p;
    std::vector<uint8_t> blob((size_t)total), hv((size_t)n, 0);
    std::vector<i64> at((size_t)n);
    i64 run = 0;
    for (i64 k = 0; k < n; k++) {
        at[(size_t)k] = s.bytes + run;
        if (len[k]) memcpy(blob.data() + run, bytes + off[k], (size_t)len[k]);
        run += len[k];
        hv[(size_t)k] = half && half[k] ? 1 : 0;
    }
    HIP_TRY(c, hipMemcpyAsync(g + o_len, len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(g + o_err, 0, 8, st));
    hipLaunchKernelGGL(k_seq_put_check, dim3(div_up(n, 256)), dim3(256), 0, st, dp<i64>(s.off), dp<int>(c->pool.aux), d_rows, (const int*)(g + o_len), n, (int*)(g + o_err));
    HIP_TRY(c, hipGetLastError());
    int e = 0;
    HIP_TRY(c, hipMemcpyAsync(&e, g + o_err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (e) return fail(c, CSV_E_INVALID, "csv_seq_pool_put: %s", (e & SEQ_ERR_TAKEN) ? seq_why(SEQ_ERR_TAKEN) : "a sequence's length is not its row's aux");
    TRY(grow_keep(c, s.blob, (size_t)(s.bytes + total) + 8, (size_t)s.bytes));
    if (total) HIP_TRY(c, hipMemcpyAsync(dp<uint8_t>(s.blob) + s.bytes, blob.data(), (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(g + o_at, at.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(g + o_half, hv.data(), (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_seq_put_apply, dim3(div_up(n, 256)), dim3(256), 0, st, SeqPool{dp<uint8_t>(s.blob), dp<i64>(s.off), dp<uint8_t>(s.half)}, d_rows, (const i64*)(g + o_at),
                       (const uint8_t*)(g + o_half), n);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));                   // (the vectors are the copies' sources)
    s.bytes += total; s.n_with += n;
    return CSV_OK;
}

int csv_seq_pool_get(csv_ctx* c, int64_t n, const int32_t* pool_row, char* out, int64_t cap, int64_t* out_off)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || cap < 0 || !out_off || (n > 0 && !pool_row) || (cap > 0 && !out)) return fail(c, CSV_E_INVALID, "bad sequence pool get");
    out_off[0] = 0;
    if (n == 0) return CSV_OK;
    SeqState& s = c->seq;
    // the lengths are the pool rows' aux, which only the device holds: they come back first (4 bytes per row), the bases in one download
    const size_t o_len = (size_t)n * 4, o_off = ((o_len + (size_t)n * 4) + 7) & ~(size_t)7;
    int* d_rows = nullptr;
    TRY(seq_rows_in(c, "csv_seq_pool_get", n, pool_row, s.get, o_off + (size_t)(n + 1) * 8, &d_rows));
    hipStream_t st = c->stream;
    char* g = (char*)s.get.p;
    std::vector<int> len((size_t)n);
    hipLaunchKernelGGL(k_seq_get_len, dim3(div_up(n, 256)), dim3(256), 0, st, dp<i64>(s.off), dp<int>(c->pool.aux), d_rows, n, (int*)(g + o_len));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(len.data(), g + o_len, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (i64 k = 0; k < n; k++) {
        if (len[(size_t)k] < 0) return fail(c, CSV_E_INVALID, "csv_seq_pool_get: pool row %d has no sequence", pool_row[k]);
        out_off[k + 1] = out_off[k] + len[(size_t)k];
    }
    const i64 total = out_off[n];
    if (total > cap) return fail(c, CSV_E_CAPACITY, "out: %lld bytes are needed", (long long)total);
    if (total == 0) return CSV_OK;
    TRY(reserve(c, s.out, (size_t)total + 8));
    HIP_TRY(c, hipMemcpyAsync(g + o_off, out_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_seq_get, dim3(div_up(n, 4)), dim3(256), 0, st, dp<uint8_t>(s.blob), dp<i64>(s.off), d_rows, (const i64*)(g + o_off), n, dp<uint8_t>(s.out));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, s.out.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return CSV_OK;
}

int csv_seq_pool_half(csv_ctx* c, int64_t n, const int32_t* pool_row, uint8_t* half)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || (n > 0 && (!pool_row || !half))) return fail(c, CSV_E_INVALID, "bad sequence pool half");
    if (n == 0) return CSV_OK;
    SeqState& s = c->seq;
    for (i64 k = 0; k < n; k++)
        if (pool_row[k] < 0 || pool_row[k] >= c->pool.n) return fail(c, CSV_E_INVALID, "csv_seq_pool_half: pool_row[%lld] = %d is outside the %lld rows of the pool", (long long)k, pool_row[k], (long long)c->pool.n);
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(seq_sync(c, c->pool.n));
    std::vector<uint8_t> all((size_t)c->pool.n);            // (a byte per pool row: the whole column is smaller than a gather's round trips)
    HIP_TRY(c, hipMemcpyAsync(all.data(), s.half.p, (size_t)c->pool.n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (i64 k = 0; k < n; k++) half[k] = all[(size_t)pool_row[k]];
    return CSV_OK;
}

// CSV_RB_TIES_FROM_SEQS: the answer csv_tie_order_fn would give for the groups [goff[g], goff[g + 1]) of the pool rows `src`, made on
// the device from the sequence pool: only order[] and drop[] come back
static int seq_tie_order(csv_ctx* c, i64 n_groups, const int64_t* goff, const int32_t* src, i64 n_list, int32_t* order, uint8_t* drop)
{
    SeqState& s = c->seq;
    if (!s.off.p) return fail(c, CSV_E_INVALID, "CSV_RB_TIES_FROM_SEQS: a row of a tie group has no sequence (the context holds no sequence pool)");
    TRY(seq_sync(c, c->pool.n));
    const size_t o_src = (size_t)(n_groups + 1) * 8, o_ord = o_src + (size_t)n_list * 4, o_err = o_ord + (size_t)n_list * 4, o_drop = o_err + 8;
    TRY(reserve(c, s.tie, o_drop + (size_t)n_list + 8));
    hipStream_t st = c->stream;
    char* g = (char*)s.tie.p;
    HIP_TRY(c, hipMemcpyAsync(g, goff, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(g + o_src, src, (size_t)n_list * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(g + o_err, 0, 8, st));
    hipLaunchKernelGGL(k_seq_tie_order, dim3(div_up(n_groups, 4)), dim3(256), 0, st, dp<uint8_t>(s.blob), dp<i64>(s.off), dp<int>(c->pool.aux), dp<uint8_t>(s.half),
                       (const i64*)g, (const int*)(g + o_src), n_groups, (int*)(g + o_ord), (uint8_t*)(g + o_drop), (int*)(g + o_err));
    HIP_TRY(c, hipGetLastError());
    int e = 0;
    HIP_TRY(c, hipMemcpyAsync(order, g + o_ord, (size_t)n_list * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(drop, g + o_drop, (size_t)n_list, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&e, g + o_err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (e) return fail(c, CSV_E_INVALID, "CSV_RB_TIES_FROM_SEQS: a row of a tie group has no sequence");
    return CSV_OK;
}

int csv_seq_struct_size(int which) { return which == 0 ? (int)sizeof(csv_seq_info) : -1; }

}  // extern "C"
