// stage_names.hip.h — the device-resident name pool and its ranks (NameState in ctx.hip.h, kernels in names.hip.h):
// csv_name_pool_*, csv_name_ranks.  Host code; included by cutesv_hip.hip.
extern "C" {

int csv_name_pool_reset(csv_ctx* c)
{
    if (!c) return CSV_E_INVALID;
    c->nm.n = 0; c->nm.bytes = 0; c->nm.maxlen = 0; c->nm.len.clear();
    c->nm.fresh = false;
    c->vs.stale();
    return CSV_OK;
}

int csv_name_pool_rows(const csv_ctx* c, int64_t* n)
{
    if (!c || !n) return CSV_E_INVALID;
    *n = c->nm.n;
    return CSV_OK;
}

// csv_name_pool_append; with dev_bytes (csv_name_pool_append_framed, stage_frame.hip.h) the n_bytes bytes lie in device memory and the
// names are gathered there (k_frame_gather): what crosses the link is the offset table alone
static int name_pool_append_impl(csv_ctx* c, int64_t n, const uint8_t* bytes, const uint8_t* dev_bytes, int64_t n_bytes, const int64_t* off, const int32_t* len, int64_t* first_index)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || n_bytes < 0 || (n > 0 && (!off || !len)) || (n_bytes > 0 && !bytes && !dev_bytes)) return fail(c, CSV_E_INVALID, "bad name pool append");
    // every range is checked before the pool changes or anything is launched
    i64 total = 0; int mx = 0;
    for (i64 i = 0; i < n; i++) {
        if (len[i] < 0 || len[i] > NAME_MAX_LEN) return fail(c, CSV_E_INVALID, "name %lld: length %d is outside [0, %d]", (long long)i, len[i], NAME_MAX_LEN);
        if (off[i] < 0 || off[i] > n_bytes || (i64)len[i] > n_bytes - off[i])
            return fail(c, CSV_E_INVALID, "name %lld: bytes [%lld, %lld) leave the %lld bytes given", (long long)i, (long long)off[i], (long long)off[i] + len[i], (long long)n_bytes);
        total += len[i];
        mx = len[i] > mx ? len[i] : mx;
    }
    if (c->nm.n + n >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "name pool too large (%lld names)", (long long)(c->nm.n + n));
    if (first_index) *first_index = c->nm.n;
    if (n == 0) return CSV_OK;
    c->vs.stale();
    HIP_TRY(c, hipSetDevice(c->device));
    // the names back to back and their offsets in the pool's blob: what crosses the link (a chunk's host image also holds the bases)
    std::vector<uint8_t> blob(dev_bytes ? 0 : (size_t)total);
    std::vector<i64> offs((size_t)n + 1);
    i64 at = 0;
    for (i64 i = 0; i < n; i++) {
        offs[(size_t)i] = c->nm.bytes + at;
        if (len[i] && !dev_bytes) memcpy(blob.data() + at, bytes + off[i], (size_t)len[i]);
        at += len[i];
    }
    offs[(size_t)n] = c->nm.bytes + at;
    TRY(grow_keep(c, c->nm.blob, (size_t)(c->nm.bytes + total) + 8, (size_t)c->nm.bytes));
    TRY(grow_keep(c, c->nm.off, (size_t)(c->nm.n + n + 1) * 8, c->nm.n ? (size_t)(c->nm.n + 1) * 8 : 0));
    hipStream_t st = c->stream;
    if (total && !dev_bytes) HIP_TRY(c, hipMemcpyAsync((char*)c->nm.blob.p + c->nm.bytes, blob.data(), (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(dp<i64>(c->nm.off) + c->nm.n, offs.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if (total && dev_bytes) TRY(frame_gather(c, n, dev_bytes, off, len, dp<uint8_t>(c->nm.blob), dp<i64>(c->nm.off) + c->nm.n));
    HIP_TRY(c, hipStreamSynchronize(st));                   // (the vectors are the copies' sources)
    c->nm.len.reserve((size_t)(c->nm.n + n));
    for (i64 i = 0; i < n; i++) c->nm.len.push_back((uint8_t)len[i]);
    c->nm.n += n; c->nm.bytes += total;
    c->nm.maxlen = mx > c->nm.maxlen ? mx : c->nm.maxlen;
    c->nm.fresh = false;
    return CSV_OK;
}

int csv_name_pool_append(csv_ctx* c, int64_t n, const uint8_t* bytes, int64_t n_bytes, const int64_t* off, const int32_t* len, int64_t* first_index)
{
    return name_pool_append_impl(c, n, bytes, nullptr, n_bytes, off, len, first_index);
}

// the ranks of the pool's names into nm.rank / nm.first (nothing to do while they are fresh)
static int name_ranks_impl(csv_ctx* c)
{
    if (c->nm.fresh) return CSV_OK;
    const i64 n = c->nm.n;
    c->nm.ms = 0; c->nm.passes = 0; c->nm.distinct = 0;
    if (n == 0) { c->nm.fresh = true; return CSV_OK; }
    const int W = std::max(1, (c->nm.maxlen + 7) / 8);
    const int nunits = div_up(n, SORT_WTILE), ntile = div_up(n, NAME_TILE);
    TRY(reserve(c, c->nm.rank, (size_t)n * 4)); TRY(reserve(c, c->nm.first, (size_t)n * 4));
    Plan P;
    P.add(c->nm.words, (size_t)W * n * 8); P.add(c->nm.perm0, (size_t)n * 4); P.add(c->nm.perm1, (size_t)n * 4);
    P.add(c->nm.hist, (size_t)256 * nunits * 4); P.add(c->nm.tot, 256 * 4); P.add(c->nm.vary, (NAME_MAX_WORDS + 1) * 8);
    P.add(c->nm.flag, (size_t)n); P.add(c->nm.partial, ((size_t)ntile + 2) * 4);
    TRY(commit_synced(c, c->nm.arena, P));
    hipStream_t st = c->stream;
    u64* words = dp<u64>(c->nm.words);
    HIP_TRY(c, hipMemsetAsync(c->nm.vary.p, 0, (NAME_MAX_WORDS + 1) * 8, st));
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_name_pack, dim3(ntile, W), dim3(256), 0, st, dp<uint8_t>(c->nm.blob), dp<i64>(c->nm.off), n, words, dp<unsigned long long>(c->nm.vary));
    // the byte positions at which any two names differ: one radix pass each, least significant (the last byte of the last word) first
    unsigned long long vary[NAME_MAX_WORDS] = {};
    HIP_TRY(c, hipMemcpyAsync(vary, c->nm.vary.p, (size_t)W * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    SortField fields[NAME_MAX_WORDS];
    for (int w = W - 1, f = 0; w >= 0; w--, f++) {
        unsigned mask = 0;
        for (int byte = 0; byte < 8; byte++) if ((vary[w] >> (8 * byte)) & 255ull) mask |= 1u << byte;
        fields[f] = SortField{words + (i64)w * n, 1, 0, 8, mask};
    }
    int npass = 0;
    const int* pin = sort_passes(st, fields, W, n, nunits, dp<int>(c->nm.perm0), dp<int>(c->nm.perm1), dp<int>(c->nm.hist), dp<int>(c->nm.tot), &npass);
    int* d_n = (int*)((char*)c->nm.vary.p + NAME_MAX_WORDS * 8);
    NameRank R{n, W, words, pin, dp<uint8_t>(c->nm.flag), dp<int>(c->nm.partial), dp<int>(c->nm.rank), dp<int>(c->nm.first), d_n};
    hipLaunchKernelGGL(k_name_count, dim3(ntile), dim3(256), 0, st, R);
    hipLaunchKernelGGL(k_name_apply, dim3(ntile), dim3(256), 0, st, R);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    int nd = 0;
    HIP_TRY(c, hipMemcpyAsync(&nd, d_n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&c->nm.ms, c->ev[0], c->ev[1]));
    c->nm.distinct = nd; c->nm.passes = npass;
    c->nm.fresh = true;
    return CSV_OK;
}

int csv_name_ranks(csv_ctx* c, csv_name_rank_out* out)
{
    if (!c || !out) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(name_ranks_impl(c));
    out->n = c->nm.n; out->n_distinct = c->nm.distinct; out->ms_device = c->nm.ms; out->n_passes = c->nm.passes; out->max_len = c->nm.maxlen;
    out->dev_rank = c->nm.n ? c->nm.rank.p : nullptr;
    if (out->first && out->cap_first < c->nm.distinct) return fail(c, CSV_E_CAPACITY, "first: %lld entries are needed", (long long)c->nm.distinct);
    hipStream_t st = c->stream;
    if (out->rank && c->nm.n) HIP_TRY(c, hipMemcpyAsync(out->rank, c->nm.rank.p, (size_t)c->nm.n * 4, hipMemcpyDeviceToHost, st));
    if (out->first && c->nm.distinct) HIP_TRY(c, hipMemcpyAsync(out->first, c->nm.first.p, (size_t)c->nm.distinct * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return CSV_OK;
}

int csv_name_pool_get(csv_ctx* c, int64_t n, const int32_t* index, char* out, int64_t cap, int64_t* out_off)
{
    if (!c) return CSV_E_INVALID;
    if (n < 0 || cap < 0 || !out_off || (n > 0 && !index) || (cap > 0 && !out)) return fail(c, CSV_E_INVALID, "bad name pool get");
    out_off[0] = 0;
    for (i64 k = 0; k < n; k++) {
        if (index[k] < 0 || index[k] >= c->nm.n) return fail(c, CSV_E_INVALID, "index[%lld] = %d is outside the %lld names of the pool", (long long)k, index[k], (long long)c->nm.n);
        out_off[k + 1] = out_off[k] + c->nm.len[(size_t)index[k]];
    }
    const i64 total = out_off[n];
    if (total > cap) return fail(c, CSV_E_CAPACITY, "out: %lld bytes are needed", (long long)total);
    if (n == 0 || total == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // one buffer: the gathered bytes, then (8-byte aligned) the offsets and the indices
    const size_t o_off = ((size_t)total + 7) & ~(size_t)7, o_idx = o_off + (size_t)(n + 1) * 8;
    TRY(grow_keep(c, c->nm.get, o_idx + (size_t)n * 4, 0));
    hipStream_t st = c->stream;
    char* g = (char*)c->nm.get.p;
    HIP_TRY(c, hipMemcpyAsync(g + o_off, out_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(g + o_idx, index, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_name_gather, dim3(div_up(n, 4)), dim3(256), 0, st, dp<uint8_t>(c->nm.blob), dp<i64>(c->nm.off), (const int*)(g + o_idx), (const i64*)(g + o_off), n, (uint8_t*)g);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, g, (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return CSV_OK;
}

size_t csv_name_struct_size(int which) { return which == 0 ? sizeof(csv_name_rank_out) : 0; }

}  // extern "C"
