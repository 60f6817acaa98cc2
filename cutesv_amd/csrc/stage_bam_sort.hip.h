// stage_bam_sort.hip.h — the coordinate sort of a BAM file on the device (BamSortState in ctx.hip.h; sort_core.h; k_sort_* at the end of bam.hip.h;
// DESIGN.md section 39): the reader's internal entries (csv_sort_*, declared in sort_core.h, called by bam_host.cpp alone).  The
// inflated stream is collected in one arena - device to device on the framing route, uploaded otherwise; the record starts go up
// once; what comes down is a verdict of three words and, slice by slice, the compressed blocks.  Host code; included by cutesv_hip.hip
// behind stage_index.hip.h (the slices are compressed by stage_deflate.hip.h's dfl_run where they lie).

int csv_sort_free_bytes(csv_ctx* c, int64_t* free_bytes)
{
    if (!c || !free_bytes) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    size_t fr = 0, tot = 0;
    HIP_TRY(c, hipMemGetInfo(&fr, &tot));
    *free_bytes = (int64_t)fr;
    return CSV_OK;
}

int csv_sort_begin(csv_ctx* c, int64_t arena_bytes, const uint8_t* hdr, int64_t hdr_bytes, int64_t slice_bytes)
{
    if (!c) return CSV_E_INVALID;
    BamSortState& s = c->bs;
    s.arena_bytes = -1; s.n = -1; s.order = nullptr; s.total = 0;
    if (arena_bytes < 0 || hdr_bytes < 12 || !hdr || slice_bytes < SORT_BLOCK || slice_bytes % SORT_BLOCK) return fail(c, CSV_E_INVALID, "bad sort: the arena, the header or the slice");
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(reserve(c, s.arena, (size_t)arena_bytes + 32));
    TRY(reserve(c, s.hdr, (size_t)hdr_bytes + 16));
    TRY(reserve(c, s.slice, (size_t)slice_bytes + 64));
    TRY(h2d(c, s.hdr, hdr, hdr_bytes));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    s.arena_bytes = arena_bytes; s.hdr_bytes = hdr_bytes; s.slice_bytes = slice_bytes;
    for (double& m : s.ms) m = 0;
    s.bytes_up = hdr_bytes; s.bytes_down = 0;
    return CSV_OK;
}

int csv_sort_append(csv_ctx* c, int64_t arena_off, const uint8_t* src, int64_t win_off, int64_t len)
{
    if (!c) return CSV_E_INVALID;
    BamSortState& s = c->bs;
    if (s.arena_bytes < 0) return fail(c, CSV_E_STATE, "no sort is open on this context");
    if (arena_off < 0 || len < 0 || arena_off > s.arena_bytes - len) return fail(c, CSV_E_INVALID, "bad sort: bytes outside the arena");
    if (len == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (src) {
        HIP_TRY(c, hipMemcpyAsync(dp<uint8_t>(s.arena) + arena_off, src, (size_t)len, hipMemcpyHostToDevice, c->stream));
        s.bytes_up += len;
    } else {
        const FrameState& f = c->fr;
        if (win_off < 0 || win_off > f.win_n - len) return fail(c, CSV_E_INVALID, "bad sort: bytes outside the framing window");
        HIP_TRY(c, hipMemcpyAsync(dp<uint8_t>(s.arena) + arena_off, dp<uint8_t>(f.win[f.cur]) + win_off, (size_t)len, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                               // (the source is the reader's window, which moves on)
    return CSV_OK;
}

int csv_sort_order(csv_ctx* c, int64_t n, const int64_t* starts, int32_t n_ref, csv_sort_verdict* v)
{
    if (!c || !v) return CSV_E_INVALID;
    BamSortState& s = c->bs;
    v->bad = SORT_NONE; v->inversions = 0; v->record_bytes = 0; v->passes = 0;
    if (s.arena_bytes < 0) return fail(c, CSV_E_STATE, "no sort is open on this context");
    if (n < 0 || n_ref < 0 || (n > 0 && !starts)) return fail(c, CSV_E_INVALID, "bad sort: the record table");
    if (n > (1ll << 31) - 8192) return fail(c, CSV_E_INVALID, "cannot sort: %lld records are more than the permutation's 2^31 - 8192", (long long)n);
    s.n = -1; s.order = nullptr;
    if (n == 0) { s.n = 0; s.total = 0; return CSV_OK; }
    // the kernels trust the table: every key field lies inside the arena
    for (i64 i = 0; i < n; i++)
        if (starts[i] < 0 || starts[i] > s.arena_bytes - 36) return fail(c, CSV_E_INVALID, "bad sort: record %lld starts outside the arena", (long long)i);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int nunits = div_up(n, SORT_WTILE), ntile = div_up(n, SORT_DST_TILE);
    const size_t z = (size_t)n;
    TRY(reserve(c, s.starts, 8 * z));
    TRY(reserve(c, s.key, 8 * z));
    TRY(reserve(c, s.len, 8 * z));
    TRY(reserve(c, s.perm[0], 4 * z));
    TRY(reserve(c, s.perm[1], 4 * z));
    TRY(reserve(c, s.hist, (size_t)256 * nunits * 4));
    TRY(reserve(c, s.tot, 256 * 4));
    TRY(reserve(c, s.dst, 8 * (z + 1)));
    TRY(reserve(c, s.tiles, 8 * (size_t)ntile));
    TRY(reserve(c, s.verdict, 32));
    TRY(h2d(c, s.starts, starts, 8 * n));
    const u64 v0[3] = {SORT_NONE, 0, 0};
    TRY(h2d(c, s.verdict, v0, sizeof v0));
    s.bytes_up += 8 * n;
    const SortKeyArgs K{dp<uint8_t>(s.arena), s.arena_bytes, dp<i64>(s.starts), n, n_ref, dp<u64>(s.key), dp<i64>(s.len), dp<u64>(s.verdict)};
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_sort_keys, dim3(div_up(n, 256)), dim3(256), 0, st, K);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    u64 got[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(got, s.verdict.p, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    s.ms[0] += ms; s.bytes_down += (i64)sizeof got;
    v->bad = got[0]; v->inversions = (long long)got[1];
    if (got[0] != SORT_NONE) return CSV_OK;                                    // (the caller refuses; nothing is ordered)
    // the 8-bit digits some key has a bit in, inside what n_ref allows at all: only those passes run
    const u64 live = got[2] & sort_key_bits(n_ref);
    unsigned mask = 0;
    for (int b = 0; b < 8; b++) if ((live >> (8 * b)) & 255) mask |= 1u << b;
    const SortField F{s.key.p, 1, 0, 8, mask};
    const SortDstArgs D0{dp<i64>(s.len), nullptr, n, dp<i64>(s.dst), dp<i64>(s.tiles)};
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    const int* order = sort_passes(st, &F, 1, n, nunits, dp<int>(s.perm[0]), dp<int>(s.perm[1]), dp<int>(s.hist), dp<int>(s.tot), &v->passes);
    SortDstArgs D = D0;
    D.perm = order;
    hipLaunchKernelGGL(k_sort_dst_tiles, dim3(ntile), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_sort_dst_scan, dim3(ntile), dim3(256), 0, st, D);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    i64 total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, dp<i64>(s.dst) + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    s.ms[1] += ms; s.bytes_down += 8;
    s.n = n; s.order = order; s.total = total;
    v->record_bytes = total;
    return CSV_OK;
}

int csv_sort_slice(csv_ctx* c, int64_t s0, int64_t len, uint8_t* out, int64_t out_cap, int32_t* block_bytes, int64_t* out_bytes)
{
    if (!c || !out_bytes) return CSV_E_INVALID;
    BamSortState& s = c->bs;
    *out_bytes = 0;
    if (s.arena_bytes < 0 || s.n < 0) return fail(c, CSV_E_STATE, "no ordered sort is open on this context");
    if (s0 < 0 || (s0 & 15) || len < 1 || len > s.slice_bytes || s0 > s.hdr_bytes + s.total - len || !out || !block_bytes) return fail(c, CSV_E_INVALID, "bad sort: the slice");
    const int32_t nb = (int32_t)((len + SORT_BLOCK - 1) / SORT_BLOCK);
    if (out_cap < len + 31ll * nb) return fail(c, CSV_E_INVALID, "bad sort: the slice's blocks need room for %lld bytes", (long long)(len + 31ll * nb));
    s.off_h.resize((size_t)nb); s.len_h.resize((size_t)nb);
    for (int32_t k = 0; k < nb; k++) { s.off_h[(size_t)k] = (i64)k * SORT_BLOCK; s.len_h[(size_t)k] = (int32_t)std::min<i64>(SORT_BLOCK, len - (i64)k * SORT_BLOCK); }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const SortGatherArgs G{dp<uint8_t>(s.arena), dp<uint8_t>(s.hdr), s.hdr_bytes, dp<i64>(s.starts), s.order, dp<i64>(s.dst), s.n, s0, len, dp<uint8_t>(s.slice)};
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    hipLaunchKernelGGL(k_sort_gather, dim3(div_up(div_up(len, SORT_GATHER_TILE), 4)), dim3(256), 0, st, G);
    HIP_TRY(c, hipEventRecord(c->ev[3], st));
    HIP_TRY(c, hipGetLastError());
    double ms_d = 0;
    static_assert(sizeof(i64) == sizeof(int64_t), "the block table is handed on as it is");
    TRY(dfl_run(c, dp<uint8_t>(s.slice), nullptr, len, nb, (const int64_t*)s.off_h.data(), s.len_h.data(), out, out_cap, block_bytes, out_bytes, &ms_d));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    s.ms[2] += ms; s.ms[3] += ms_d;
    s.bytes_up += 12ll * nb; s.bytes_down += *out_bytes + 4ll * nb + 8;
    return CSV_OK;
}

int csv_sort_counters(csv_ctx* c, double* ms4, int64_t* bytes_up, int64_t* bytes_down)
{
    if (!c) return CSV_E_INVALID;
    const BamSortState& s = c->bs;
    if (ms4) for (int k = 0; k < 4; k++) ms4[k] = s.ms[k];
    if (bytes_up) *bytes_up = s.bytes_up;
    if (bytes_down) *bytes_down = s.bytes_down;
    return CSV_OK;
}

int csv_sort_end(csv_ctx* c)
{
    if (!c) return CSV_E_INVALID;
    BamSortState& s = c->bs;
    s.arena_bytes = -1; s.n = -1; s.order = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (s.arena.p) { HIP_TRY(c, hipFree(s.arena.p)); s.arena.p = nullptr; s.arena.cap = 0; }
    return CSV_OK;
}
