// stage_aln.hip.h — csv_aln_*: the alignment table and the TRA genotyping over it (AlnState in ctx.hip.h, kernels in aln.hip.h,
// DESIGN.md section 18).  Host code; included by cutesv_hip.hip.

// what both appends check first
static int aln_append_args(csv_ctx* c, const char* what, int chrom, i64 upper)
{
    AlnState& a = c->al;
    if (chrom < 0 || chrom >= a.n_chrom) return fail(c, CSV_E_INVALID, "%s: chromosome %d is outside the %d of csv_aln_reset", what, chrom, a.n_chrom);
    if (chrom < a.last_chrom) return fail(c, CSV_E_UNSORTED, "%s: chromosome %d comes after rows of chromosome %d", what, chrom, a.last_chrom);
    if (a.n + upper >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "%s: alignment table too large (%lld rows)", what, (long long)(a.n + upper));
    return CSV_OK;
}

// room for `upper` more rows, the frame of the kernels' arguments, the pending words cleared (at the head of al.work)
static int aln_begin(csv_ctx* c, int chrom, i64 upper, size_t work_bytes, AlnAppend* A)
{
    AlnState& a = c->al;
    TRY(grow_keep(c, a.start, (size_t)(a.n + upper) * 4, (size_t)a.n * 4));
    TRY(grow_keep(c, a.end, (size_t)(a.n + upper) * 4, (size_t)a.n * 4));
    TRY(grow_keep(c, a.idp, (size_t)(a.n + upper) * 4, (size_t)a.n * 4));
    TRY(reserve(c, a.work, work_bytes));
    HIP_TRY(c, hipMemsetAsync(a.work.p, 0, 128, c->stream));
    A->T = AlnCols{dp<int>(a.start), dp<int>(a.end), dp<int>(a.idp)};
    A->n0 = a.n; A->prev_same = (a.n > 0 && a.last_chrom == chrom) ? 1 : 0; A->chrom = chrom;
    A->maxlen = dp<int>(a.maxlen); A->pend = dp<int>(a.work);
    return CSV_OK;
}

// the new rows (at most `upper`) lie behind the table: order check, longest record, and - when all is well - the count moves
static int aln_commit(csv_ctx* c, const char* what, const AlnAppend& A, i64 upper, i64 max_id, int64_t* n_appended)
{
    AlnState& a = c->al;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_aln_check, dim3(div_up(upper, 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_aln_apply, dim3(1), dim3(64), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    int pend[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(pend, A.pend, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&a.ms_append, c->ev[0], c->ev[1]));
    if (pend[0]) return fail(c, CSV_E_UNSORTED, "%s: the starts do not ascend inside chromosome %d", what, A.chrom);
    const i64 m = pend[2];
    if (m < 0 || m > upper) return fail(c, CSV_E_INVALID, "%s: inconsistent row count %lld", what, (long long)m);
    if (n_appended) *n_appended = m;
    if (m == 0) return CSV_OK;
    a.n += m; a.last_chrom = A.chrom;
    a.max_id = std::max(a.max_id, max_id);
    for (int k = A.chrom + 1; k <= a.n_chrom; k++) a.h_off[(size_t)k] += m;
    return CSV_OK;
}

extern "C" {

int csv_aln_reset(csv_ctx* c, int32_t n_chrom)
{
    if (!c) return CSV_E_INVALID;
    if (n_chrom < 0 || n_chrom > (1 << 24)) return fail(c, CSV_E_INVALID, "csv_aln_reset: %d chromosomes", n_chrom);
    HIP_TRY(c, hipSetDevice(c->device));
    AlnState& a = c->al;
    TRY(reserve(c, a.maxlen, (size_t)(n_chrom + 1) * 4));
    HIP_TRY(c, hipMemsetAsync(a.maxlen.p, 0, (size_t)(n_chrom + 1) * 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    a.n = 0; a.max_id = -1; a.n_chrom = n_chrom; a.last_chrom = -1;
    a.h_off.assign((size_t)n_chrom + 1, 0);
    return CSV_OK;
}

int csv_aln_rows(const csv_ctx* c, int64_t* n)
{
    if (!c || !n) return CSV_E_INVALID;
    *n = c->al.n;
    return CSV_OK;
}

int csv_aln_append_decoded(csv_ctx* c, int32_t chrom, int64_t beg, int64_t end, int64_t name_base, int64_t* n_appended)
{
    if (!c) return CSV_E_INVALID;
    if (n_appended) *n_appended = 0;
    const i64 n = c->bm.n;
    if (n < 0) return fail(c, CSV_E_INVALID, "csv_aln_append_decoded: the context holds no decoded BAM chunk");
    if (beg < 0 || end < beg) return fail(c, CSV_E_INVALID, "csv_aln_append_decoded: bad range [%lld, %lld)", (long long)beg, (long long)end);
    if (name_base < 0 || name_base + n >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "csv_aln_append_decoded: name ids %lld .. leave 31 bits", (long long)name_base);
    TRY(aln_append_args(c, "csv_aln_append_decoded", chrom, n));
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // work: pending words and the scan's totals (128 bytes, cleared), per record {keep -> offset}, the tile sums
    const size_t o_cnt = 128, o_tiles = o_cnt + (((size_t)(n + 1) * 16 + 255) & ~(size_t)255);
    AlnAppend A{};
    TRY(aln_begin(c, chrom, n, o_tiles + scan_tile_bytes(n) + 64, &A));
    char* g = (char*)c->al.work.p;
    i64* tot = (i64*)(g + 64);
    int4* cnt = (int4*)(g + o_cnt);
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_aln_keep, dim3(div_up(n, 256)), dim3(256), 0, st, dp<i64>(c->bm.start), n, (i64)beg, (i64)end, cnt);
    scan_counts(st, ScanArgs{n, cnt, (i64*)(g + o_tiles), tot});   // the keep flags' exclusive prefix
    hipLaunchKernelGGL(k_aln_store, dim3(div_up(n, 256)), dim3(256), 0, st, A, dp<i64>(c->bm.start), dp<i64>(c->bm.end), dp<int>(c->bm.flag), n, (i64)beg, (i64)end, (int)name_base,
                       cnt, tot);
    return aln_commit(c, "csv_aln_append_decoded", A, n, name_base + n - 1, n_appended);
}

int csv_aln_append(csv_ctx* c, int32_t chrom, int64_t n, const int32_t* start, const int32_t* end, const uint8_t* primary, const int32_t* id)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || (n > 0 && (!start || !end || !primary || !id))) return fail(c, CSV_E_INVALID, "bad alignment append");
    TRY(aln_append_args(c, "csv_aln_append", chrom, n));
    i64 max_id = -1;
    for (i64 i = 0; i < n; i++) {
        if (start[i] < 0 || end[i] <= start[i] || id[i] < 0)
            return fail(c, CSV_E_INVALID, "csv_aln_append: row %lld (start %d, end %d, id %d): 0 <= start < end and id >= 0 are expected", (long long)i, start[i], end[i], id[i]);
        max_id = std::max<i64>(max_id, id[i]);
    }
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t o_s = 128, o_e = o_s + (size_t)n * 4, o_i = o_e + (size_t)n * 4, o_p = o_i + (size_t)n * 4;
    AlnAppend A{};
    TRY(aln_begin(c, chrom, n, o_p + (size_t)n + 64, &A));
    char* g = (char*)c->al.work.p;
    HIP_TRY(c, hipMemcpyAsync(g + o_s, start, (size_t)n * 4, hipMemcpyHostToDevice, st)); HIP_TRY(c, hipMemcpyAsync(g + o_e, end, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(g + o_i, id, (size_t)n * 4, hipMemcpyHostToDevice, st)); HIP_TRY(c, hipMemcpyAsync(g + o_p, primary, (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_aln_put, dim3(div_up(n, 256)), dim3(256), 0, st, A, (const int*)(g + o_s), (const int*)(g + o_e), (const uint8_t*)(g + o_p), (const int*)(g + o_i), (i64)n);
    return aln_commit(c, "csv_aln_append", A, n, max_id, nullptr);
}

int csv_aln_get(csv_ctx* c, int64_t first, int64_t n, int32_t* start, int32_t* end, uint8_t* primary, int32_t* id)
{
    if (!c) return CSV_E_INVALID;
    if (first < 0 || n < 0 || first > c->al.n || n > c->al.n - first) return fail(c, CSV_E_INVALID, "csv_aln_get: rows [%lld, %lld) of %lld", (long long)first, (long long)(first + n), (long long)c->al.n);
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<int> idp((size_t)n);
    if (start) HIP_TRY(c, hipMemcpyAsync(start, dp<int>(c->al.start) + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (end) HIP_TRY(c, hipMemcpyAsync(end, dp<int>(c->al.end) + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(idp.data(), dp<int>(c->al.idp) + first, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (i64 i = 0; i < n; i++) {
        if (primary) primary[i] = idp[(size_t)i] < 0 ? 1 : 0;
        if (id) id[i] = idp[(size_t)i] & 0x7fffffff;
    }
    return CSV_OK;
}

int csv_aln_layout(csv_ctx* c, int32_t n_chrom, int64_t* off, int32_t* maxlen)
{
    if (!c) return CSV_E_INVALID;
    if (n_chrom != c->al.n_chrom) return fail(c, CSV_E_INVALID, "csv_aln_layout: %d chromosomes, the table has %d", n_chrom, c->al.n_chrom);
    if (off) for (int k = 0; k <= n_chrom; k++) off[k] = c->al.h_off[(size_t)k];
    if (maxlen && n_chrom > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemcpyAsync(maxlen, c->al.maxlen.p, (size_t)n_chrom * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return CSV_OK;
}

int csv_aln_timing(const csv_ctx* c, float* ms_append, float* ms_genotype)
{
    if (!c) return CSV_E_INVALID;
    if (ms_append) *ms_append = c->al.ms_append;
    if (ms_genotype) *ms_genotype = c->al.ms_genotype;
    return CSV_OK;
}

int csv_aln_tra_genotype(csv_ctx* c, int64_t n_calls, const int32_t* chrom1, const int64_t* pos1, const int32_t* chrom2, const int64_t* pos2, const int64_t* support_off,
                         const void* support, int32_t flags, int32_t n_chrom, const int64_t* contig_len, int64_t bias, int64_t gt_round, int32_t* out_dr, int32_t* out_status)
{
    if (!c) return CSV_E_INVALID;
    const char* what = "csv_aln_tra_genotype";
    AlnState& a = c->al;
    if (n_calls < 0 || !support_off || (flags & ~(CSV_ALN_FROM_KEPT_REBUILD | CSV_ALN_SUPPORT_I32)) || bias < 0 ||
        (n_calls > 0 && (!chrom1 || !pos1 || !chrom2 || !pos2 || !contig_len || !out_dr || !out_status)))
        return fail(c, CSV_E_INVALID, "bad TRA genotype call");
    if (n_calls >= (1ll << 30)) return fail(c, CSV_E_INVALID, "%s: too many calls (%lld): split the batch", what, (long long)n_calls);
    if (n_chrom != a.n_chrom) return fail(c, CSV_E_INVALID, "%s: %d chromosomes, the alignment table has %d", what, n_chrom, a.n_chrom);
    const bool by_rank = (flags & CSV_ALN_FROM_KEPT_REBUILD) != 0, narrow = (flags & CSV_ALN_SUPPORT_I32) != 0;
    if (by_rank) {
        TRY(vs_ready(c, what));
        if (!c->vs.by_name || !c->nm.fresh) return fail(c, CSV_E_INVALID, "%s: the kept rebuild's read ids are not ranks of the name pool (CSV_RB_RANK_FROM_NAMES)", what);
        if (a.max_id >= c->nm.n) return fail(c, CSV_E_INVALID, "%s: the table holds name id %lld, the name pool %lld names", what, (long long)a.max_id, (long long)c->nm.n);
    }
    // the offsets, every support and every chromosome are checked before anything is launched
    if (support_off[0] != 0) return fail(c, CSV_E_INVALID, "%s: support_off must start at 0", what);
    for (i64 k = 0; k < n_calls; k++) {
        if (support_off[k + 1] < support_off[k]) return fail(c, CSV_E_INVALID, "%s: support_off decreases at call %lld", what, (long long)k);
        if (chrom1[k] < 0 || chrom1[k] >= n_chrom || chrom2[k] < 0 || chrom2[k] >= n_chrom)
            return fail(c, CSV_E_INVALID, "%s: call %lld lies on chromosomes %d / %d of %d", what, (long long)k, chrom1[k], chrom2[k], n_chrom);
    }
    const i64 ns = support_off[n_calls];
    if (ns >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "%s: too many supports (%lld): split the batch", what, (long long)ns);
    if (ns > 0 && !support) return fail(c, CSV_E_INVALID, "bad TRA genotype call");
    const i64 sup_end = by_rank ? c->vs.n_out : (1ll << 31);
    // the calls whose name set does not fit the 4 096 LDS slots get a slice of global memory each
    std::vector<int> big;
    std::vector<i64> big_off;
    i64 gset = 0;
    for (i64 k = 0; k < n_calls; k++) {
        const int bits = tra_bits_for(support_off[k + 1] - support_off[k]);
        if (bits <= 12) continue;
        big.push_back((int)k); big_off.push_back(gset);
        gset += 2ll << bits;
        if (gset >= (1ll << 31)) return fail(c, CSV_E_INVALID, "%s: the name sets of the large calls need %lld slots: split the batch", what, (long long)gset);
    }
    const i64 nb = (i64)big.size();
    // one image of the call tables: the 64-bit columns first
    const size_t o_pos1 = 0, o_pos2 = o_pos1 + (size_t)n_calls * 8, o_soff = o_pos2 + (size_t)n_calls * 8, o_clen = o_soff + (size_t)(n_calls + 1) * 8,
                 o_boff = o_clen + (size_t)n_chrom * 8, o_off = o_boff + (size_t)nb * 8, o_c1 = o_off + (size_t)(n_chrom + 1) * 8, o_c2 = o_c1 + (size_t)n_calls * 4,
                 o_big = o_c2 + (size_t)n_calls * 4, o_sup = o_big + (size_t)nb * 4, o_end = o_sup + (size_t)ns * 4;
    std::vector<char> img(o_end + 8);
    int* sup = (int*)(img.data() + o_sup);
    for (i64 j = 0; j < ns; j++) {
        const i64 v = narrow ? ((const int32_t*)support)[j] : ((const int64_t*)support)[j];
        if (v < 0 || v >= sup_end) return fail(c, CSV_E_INVALID, "%s: support %lld = %lld is outside [0, %lld)", what, (long long)j, (long long)v, (long long)sup_end);
        sup[j] = (int)v;
    }
    if (n_calls == 0) return CSV_OK;
    memcpy(img.data() + o_pos1, pos1, (size_t)n_calls * 8); memcpy(img.data() + o_pos2, pos2, (size_t)n_calls * 8);
    memcpy(img.data() + o_soff, support_off, (size_t)(n_calls + 1) * 8); memcpy(img.data() + o_clen, contig_len, (size_t)n_chrom * 8);
    if (nb) { memcpy(img.data() + o_boff, big_off.data(), (size_t)nb * 8); memcpy(img.data() + o_big, big.data(), (size_t)nb * 4); }
    memcpy(img.data() + o_off, a.h_off.data(), (size_t)(n_chrom + 1) * 8);
    memcpy(img.data() + o_c1, chrom1, (size_t)n_calls * 4); memcpy(img.data() + o_c2, chrom2, (size_t)n_calls * 4);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // gt: the image, then the results {dr, status} and the error word, then the global sets
    const size_t o_res = (o_end + 255) & ~(size_t)255, o_err = o_res + (size_t)n_calls * 8, o_gset = (o_err + 64 + 255) & ~(size_t)255;
    TRY(reserve(c, a.gt, o_gset + (size_t)gset * 4 + 64));
    char* g = (char*)a.gt.p;
    HIP_TRY(c, hipMemcpyAsync(g, img.data(), o_end, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(g + o_err, 0, 64, st));
    TraAln A{};
    A.start = dp<int>(a.start); A.end = dp<int>(a.end); A.idp = dp<int>(a.idp);
    A.off = (const i64*)(g + o_off); A.maxlen = dp<int>(a.maxlen); A.contig_len = (const i64*)(g + o_clen);
    A.rank = by_rank ? dp<int>(c->nm.rank) : nullptr; A.rid = by_rank ? dp<int>(c->rb.orid) : nullptr;
    A.n_calls = (int)n_calls; A.chrom1 = (const int*)(g + o_c1); A.chrom2 = (const int*)(g + o_c2); A.pos1 = (const i64*)(g + o_pos1); A.pos2 = (const i64*)(g + o_pos2);
    A.sup_off = (const i64*)(g + o_soff); A.sup = (const int*)(g + o_sup); A.bias = bias; A.gt_round = gt_round;
    A.out_dr = (int*)(g + o_res); A.out_status = A.out_dr + n_calls; A.err = (int*)(g + o_err);
    A.n_big = (int)nb; A.big_list = (const int*)(g + o_big); A.big_off = (const i64*)(g + o_boff); A.gset = (int*)(g + o_gset);
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    if (nb < n_calls) hipLaunchKernelGGL(k_tra_aln<false>, dim3((unsigned)std::min<i64>(n_calls, 4096)), dim3(64), 0, st, A);
    if (nb > 0) hipLaunchKernelGGL(k_tra_aln<true>, dim3((unsigned)std::min<i64>(nb, 1024)), dim3(64), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    std::vector<int> res((size_t)n_calls * 2);
    int err = 0;
    HIP_TRY(c, hipMemcpyAsync(res.data(), g + o_res, (size_t)n_calls * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&err, g + o_err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));                       // (the image was the upload's source)
    HIP_TRY(c, hipEventElapsedTime(&a.ms_genotype, c->ev[0], c->ev[1]));
    if (err) return fail(c, CSV_E_INVALID, "%s: a name set overflowed", what);
    memcpy(out_dr, res.data(), (size_t)n_calls * 4); memcpy(out_status, res.data() + n_calls, (size_t)n_calls * 4);
    return CSV_OK;
}

}  // extern "C"
