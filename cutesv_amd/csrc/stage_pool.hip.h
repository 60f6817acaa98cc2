// stage_pool.hip.h — the device-resident signature pool (PoolState in ctx.hip.h): csv_pool_*, and the attach step of the
// entries that append rows on the device.  Host code; included by cutesv_hip.hip.
extern "C" {

// the row arrays of the sequence pool (SeqState: off, half) with room for `rows` pool rows; the first c->seq.rows entries survive
static int seq_rows_reserve(csv_ctx* c, i64 rows)
{
    if (rows <= c->seq.rows_cap) return CSV_OK;
    TRY(grow_keep(c, c->seq.off, (size_t)rows * 8, (size_t)c->seq.rows * 8));
    TRY(grow_keep(c, c->seq.half, (size_t)rows, (size_t)c->seq.rows));
    c->seq.rows_cap = rows;
    return CSV_OK;
}

// room for `extra` more rows in the pool (grows by copying: the pool is not in an arena)
static int pool_reserve(csv_ctx* c, i64 extra)
{
    const i64 need = c->pool.n + extra;
    if (need <= c->pool.cap) return CSV_OK;
    if (need >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "signature pool too large (%lld rows)", (long long)need);
    const i64 cap = need + need / 2 + 4096;
    Buf* cols[5] = {&c->pool.seg, &c->pool.a, &c->pool.b, &c->pool.read, &c->pool.aux};
    const size_t w[5] = {4, 8, 8, 4, 4};
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 5; k++) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, (size_t)cap * w[k]);
        if (e != hipSuccess) return fail(c, CSV_E_NOMEM, "hipMalloc(%zu) for the signature pool failed: %s", (size_t)cap * w[k], hipGetErrorString(e));
        if (c->pool.n > 0) HIP_TRY(c, hipMemcpy(p, cols[k]->p, (size_t)c->pool.n * w[k], hipMemcpyDeviceToDevice));
        if (cols[k]->p) HIP_TRY(c, hipFree(cols[k]->p));
        cols[k]->p = p; cols[k]->cap = (size_t)cap * w[k];
    }
    c->pool.cap = cap;
    if (c->seq.off.p) TRY(seq_rows_reserve(c, cap));         // (a context that never held a sequence pays nothing)
    return CSV_OK;
}

// The attach step of an entry that appends `rows` rows on the device (CSV_CG_TO_POOL): their read indices read_base + [0, n_reads) must fit
// 31 bits; room is made and PC names the columns.  The entry launches its kernel with base row c->pool.n and adds `rows` once the launch went through.
static int pool_attach(csv_ctx* c, i64 read_base, i64 n_reads, i64 rows, PoolCols* PC)
{
    if (read_base < 0 || read_base + n_reads >= (1ll << 31)) return fail(c, CSV_E_INVALID, "read_base out of range");
    TRY(pool_reserve(c, rows));
    *PC = PoolCols{dp<int>(c->pool.seg), dp<i64>(c->pool.a), dp<i64>(c->pool.b), dp<int>(c->pool.read), dp<int>(c->pool.aux)};
    return CSV_OK;
}

int csv_pool_reset(csv_ctx* c)
{
    if (!c) return CSV_E_INVALID;
    c->pool.n = 0;
    c->vs.stale();
    c->seq.rows = 0; c->seq.bytes = 0; c->seq.n_with = 0;    // the sequence pool shadows the rows
    return CSV_OK;
}

int csv_pool_rows(const csv_ctx* c, int64_t* n_rows)
{
    if (!c || !n_rows) return CSV_E_INVALID;
    *n_rows = c->pool.n;
    return CSV_OK;
}

int csv_pool_append(csv_ctx* c, int64_t n, const int32_t* seg_id, const int64_t* a, const int64_t* b, const int32_t* read, const int32_t* aux)
{
    if (!c || n < 0 || (n > 0 && (!seg_id || !a || !b || !read || !aux))) return CSV_E_INVALID;
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->vs.stale();
    TRY(pool_reserve(c, n));
    hipStream_t st = c->stream;
    const i64 o = c->pool.n;
    const struct { Buf& col; const void* src; size_t w; } cols[5] = {{c->pool.seg, seg_id, 4}, {c->pool.a, a, 8}, {c->pool.b, b, 8}, {c->pool.read, read, 4}, {c->pool.aux, aux, 4}};
    for (const auto& k : cols) HIP_TRY(c, hipMemcpyAsync((char*)k.col.p + (size_t)o * k.w, k.src, (size_t)n * k.w, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));                   // (the caller's arrays may be pageable and are free again on return)
    c->pool.n += n;
    return CSV_OK;
}

}  // extern "C"
