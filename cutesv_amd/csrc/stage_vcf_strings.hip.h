// stage_vcf_strings.hip.h — csv_seq_alt_gather, csv_name_support_join: the ALT bases of INS calls and the RNAMES text of calls, gathered on the
// device from the last kept pool rebuild and the pools it numbers (VcfStrState in ctx.hip.h, kernels in vcf_strings.hip.h).  Host code;
// included by cutesv_hip.hip.

// may the two entries run?  Only on the sorted columns of a kept pool rebuild nothing has touched since (VcfStrState::gen)
static int vs_ready(csv_ctx* c, const char* what)
{
    if (c->vs.kept == 0) return fail(c, CSV_E_INVALID, "%s: the context holds no kept pool rebuild (CSV_RB_FROM_POOL | CSV_RB_KEEP_ON_DEVICE)", what);
    if (c->vs.kept != c->vs.gen) return fail(c, CSV_E_INVALID, "%s: the pool, the name pool or the scratch arena changed after the kept rebuild: rebuild again", what);
    return CSV_OK;
}

// The skeleton of both entries.  n_items entries (picks / supports) get a length each, n_off + 1 offsets go back to the caller
// (n_off = picks / calls).  front: bytes of the entry's own tables at the head of vs.work, which upload(base) fills;
// plan(base, cnt, err) launches the length kernel, offsets(base, cnt, tot, off64) the kernel that makes the caller's offsets
// from the scanned lengths, copy(base, cnt, blob) the copy kernel.  Nothing is written to `out` unless everything is in order.
// dev_dst (nullable): the blob is made in THAT buffer and stays there - no capacity to judge, no copy to `out` (csv_vcf_emit_device
// reads it where it lies); without it the blob passes through vs.out on its way to the host.
template <class UploadFn, class PlanFn, class OffFn, class CopyFn>
static int vs_gather(csv_ctx* c, const char* what, i64 n_items, i64 n_off, size_t front, UploadFn upload, PlanFn plan, OffFn offsets, CopyFn copy, char* out, i64 cap,
                     int64_t* out_off, Buf* dev_dst)
{
    VcfStrState& v = c->vs;
    hipStream_t st = c->stream;
    const size_t o_cnt = (front + 255) & ~(size_t)255, o_tiles = o_cnt + (((size_t)(n_items + 1) * 16 + 255) & ~(size_t)255), o_tot = o_tiles + ((scan_tile_bytes(n_items) + 255) & ~(size_t)255),
                 o_off = o_tot + 64;
    TRY(reserve(c, v.work, o_off + (size_t)(n_off + 1) * 8 + 64));
    char* g = (char*)v.work.p;
    int4* cnt = (int4*)(g + o_cnt);
    i64* tot = (i64*)(g + o_tot);
    int* err = (int*)(tot + 4);
    TRY(upload(g));
    HIP_TRY(c, hipMemsetAsync(tot, 0, 40, st));
    plan(g, cnt, err);
    scan_counts(st, ScanArgs{n_items, cnt, (i64*)(g + o_tiles), tot});   // the lengths' exclusive prefix
    offsets(g, cnt, tot, (i64*)(g + o_off));
    HIP_TRY(c, hipGetLastError());
    i64 got[5] = {0, 0, 0, 0, 0};
    std::vector<i64> off((size_t)n_off + 1);
    HIP_TRY(c, hipMemcpyAsync(got, tot, 40, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(off.data(), g + o_off, (size_t)(n_off + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));                       // (the caller's vectors were the uploads' sources)
    const int e = (int)(got[4] & 0xffffffffll);
    if (e) return fail(c, CSV_E_INVALID, "%s: %s", what, (e & VS_ERR_NO_SEQ) ? "a picked row has no sequence (not an INS row of the sequence pool)" : "a support's read id is no rank of the name pool");
    if (got[0] < 0 || got[0] >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "%s: %lld bytes in one call: split the batch", what, (long long)got[0]);
    memcpy(out_off, off.data(), (size_t)(n_off + 1) * 8);
    const i64 need = out_off[n_off];
    if (!dev_dst && need > cap) return fail(c, CSV_E_CAPACITY, "out: %lld bytes are needed", (long long)need);
    if (need == 0) return CSV_OK;
    Buf& dst = dev_dst ? *dev_dst : v.out;
    TRY(reserve(c, dst, (size_t)need + 8));
    copy(g, cnt, dp<uint8_t>(dst));
    HIP_TRY(c, hipGetLastError());
    if (dev_dst) return CSV_OK;
    HIP_TRY(c, hipMemcpyAsync(out, v.out.p, (size_t)need, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return CSV_OK;
}

// grids: one thread / one wavefront per entry up to a cap; the kernels stride over what is left
static int vs_grid_threads(i64 n) { return std::max(1, std::min(div_up(n, 256), 65536)); }
static int vs_grid_waves(i64 n) { return std::max(1, std::min(div_up(n, 4), 8192)); }

// the bodies of the two entries; dev_dst: vs_gather's
static int alt_gather_run(csv_ctx* c, int64_t n, const void* pick, const void* clip, int32_t flags, char* out, int64_t cap, int64_t* out_off, Buf* dev_dst)
{
    if (n < 0 || cap < 0 || !out_off || (n > 0 && (!pick || !clip)) || (cap > 0 && !out) || (flags & ~CSV_OUT_COORD_I32)) return fail(c, CSV_E_INVALID, "bad alt gather");
    if (n >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "csv_seq_alt_gather: too many picks (%lld): split the batch", (long long)n);
    TRY(vs_ready(c, "csv_seq_alt_gather"));
    // every pick and every clip is checked before anything is launched; both cross the link as 32-bit words (a row's aux is one)
    const bool narrow = (flags & CSV_OUT_COORD_I32) != 0;
    std::vector<int> rows((size_t)n), clips((size_t)n);
    for (i64 k = 0; k < n; k++) {
        const i64 p = narrow ? ((const int32_t*)pick)[k] : ((const int64_t*)pick)[k], cl = narrow ? ((const int32_t*)clip)[k] : ((const int64_t*)clip)[k];
        if (p < 0 || p >= c->vs.n_out) return fail(c, CSV_E_INVALID, "csv_seq_alt_gather: pick[%lld] = %lld is outside the %lld rows of the rebuild", (long long)k, (long long)p, (long long)c->vs.n_out);
        if (cl < 0) return fail(c, CSV_E_INVALID, "csv_seq_alt_gather: clip[%lld] = %lld is negative", (long long)k, (long long)cl);
        rows[(size_t)k] = (int)p; clips[(size_t)k] = (int)std::min<i64>(cl, 0x7fffffff);
    }
    out_off[0] = 0;
    if (n == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    SeqState& s = c->seq;
    if (!s.off.p) return fail(c, CSV_E_INVALID, "csv_seq_alt_gather: a picked row has no sequence (the context holds no sequence pool)");
    TRY(seq_sync(c, c->pool.n));
    hipStream_t st = c->stream;
    const VsRows R{dp<int>(c->rb.osrc), dp<int>(c->rb.orid), dp<int>(c->rb.oaux)};
    const size_t o_clip = (size_t)n * 4;
    return vs_gather(c, "csv_seq_alt_gather", n, n, (size_t)n * 8,
        [&](char* g) { HIP_TRY(c, hipMemcpyAsync(g, rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, st)); HIP_TRY(c, hipMemcpyAsync(g + o_clip, clips.data(), (size_t)n * 4, hipMemcpyHostToDevice, st)); return (int)CSV_OK; },
        [&](char* g, int4* cnt, int* err) { hipLaunchKernelGGL(k_alt_plan, dim3(vs_grid_threads(n)), dim3(256), 0, st, R, dp<i64>(s.off), (const int*)g, (const int*)(g + o_clip), n, cnt, err); },
        [&](char*, int4* cnt, i64* tot, i64* off) { hipLaunchKernelGGL(k_vs_offsets, dim3(vs_grid_threads(n + 1)), dim3(256), 0, st, cnt, tot, n, off); },
        [&](char* g, int4* cnt, uint8_t* blob) { hipLaunchKernelGGL(k_alt_copy, dim3(vs_grid_waves(n)), dim3(256), 0, st, R, dp<uint8_t>(s.blob), dp<i64>(s.off), (const int*)g, (const int*)(g + o_clip), n, cnt, blob); },
        out, cap, out_off, dev_dst);
}

static int support_join_run(csv_ctx* c, int64_t n_calls, const int64_t* support_off, const int64_t* support_sig, const int32_t* support_sig32, char* out, int64_t cap, int64_t* out_off,
                            Buf* dev_dst)
{
    if (n_calls < 0 || cap < 0 || !out_off || !support_off || (cap > 0 && !out) || (support_sig && support_sig32)) return fail(c, CSV_E_INVALID, "bad support join");
    if (n_calls >= (1ll << 30)) return fail(c, CSV_E_INVALID, "csv_name_support_join: too many calls (%lld): split the batch", (long long)n_calls);
    TRY(vs_ready(c, "csv_name_support_join"));
    if (!c->vs.by_name || !c->nm.fresh) return fail(c, CSV_E_INVALID, "csv_name_support_join: the kept rebuild's read ids are not ranks of the name pool (CSV_RB_RANK_FROM_NAMES)");
    // the offsets and every support are checked before anything is launched
    if (support_off[0] != 0) return fail(c, CSV_E_INVALID, "csv_name_support_join: support_off must start at 0");
    for (i64 k = 0; k < n_calls; k++)
        if (support_off[k + 1] < support_off[k]) return fail(c, CSV_E_INVALID, "csv_name_support_join: support_off decreases at call %lld", (long long)k);
    const i64 ns = support_off[n_calls];
    if (ns >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "csv_name_support_join: too many supports (%lld): split the batch", (long long)ns);
    if (ns > 0 && !support_sig && !support_sig32) return fail(c, CSV_E_INVALID, "bad support join");
    // per support: its row, and (non-empty calls in front of its call) << 1 | it is the last of its call; per call: the same count
    std::vector<int> sup((size_t)ns), adj((size_t)ns);
    std::vector<i64> before((size_t)n_calls + 1);
    i64 nonempty = 0;
    for (i64 k = 0; k < n_calls; k++) {
        before[(size_t)k] = nonempty;
        for (i64 j = support_off[k]; j < support_off[k + 1]; j++) {
            const i64 sg = support_sig ? support_sig[j] : support_sig32[j];
            if (sg < 0 || sg >= c->vs.n_out) return fail(c, CSV_E_INVALID, "csv_name_support_join: support %lld = %lld is outside the %lld rows of the rebuild", (long long)j, (long long)sg, (long long)c->vs.n_out);
            sup[(size_t)j] = (int)sg; adj[(size_t)j] = (int)(nonempty << 1) | (j + 1 == support_off[k + 1] ? 1 : 0);
        }
        nonempty += support_off[k + 1] > support_off[k] ? 1 : 0;
    }
    before[(size_t)n_calls] = nonempty;
    for (i64 k = 0; k <= n_calls; k++) out_off[k] = 0;
    if (ns == 0) return CSV_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const VsRows R{dp<int>(c->rb.osrc), dp<int>(c->rb.orid), dp<int>(c->rb.oaux)};
    const VsNames N{dp<uint8_t>(c->nm.blob), dp<i64>(c->nm.off), dp<int>(c->nm.first), c->nm.distinct};
    // the entry's tables: supports, adj (4 bytes each), then (8-byte aligned) support_off and before
    const size_t o_adj = (size_t)ns * 4, o_soff = (o_adj + (size_t)ns * 4 + 7) & ~(size_t)7, o_bef = o_soff + (size_t)(n_calls + 1) * 8;
    return vs_gather(c, "csv_name_support_join", ns, n_calls, o_bef + (size_t)(n_calls + 1) * 8,
        [&](char* g) {
            HIP_TRY(c, hipMemcpyAsync(g, sup.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st)); HIP_TRY(c, hipMemcpyAsync(g + o_adj, adj.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(g + o_soff, support_off, (size_t)(n_calls + 1) * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(g + o_bef, before.data(), (size_t)(n_calls + 1) * 8, hipMemcpyHostToDevice, st));
            return (int)CSV_OK;
        },
        [&](char* g, int4* cnt, int* err) { hipLaunchKernelGGL(k_join_plan, dim3(vs_grid_threads(ns)), dim3(256), 0, st, R, N, (const int*)g, ns, cnt, err); },
        [&](char* g, int4* cnt, i64* tot, i64* off) { hipLaunchKernelGGL(k_join_call_off, dim3(vs_grid_threads(n_calls + 1)), dim3(256), 0, st, cnt, tot, (const i64*)(g + o_soff), (const i64*)(g + o_bef), n_calls, ns, off); },
        [&](char* g, int4* cnt, uint8_t* blob) { hipLaunchKernelGGL(k_join_copy, dim3(vs_grid_waves(ns)), dim3(256), 0, st, R, N, (const int*)g, (const int*)(g + o_adj), ns, cnt, blob); },
        out, cap, out_off, dev_dst);
}

extern "C" {

int csv_seq_alt_gather(csv_ctx* c, int64_t n, const void* pick, const void* clip, int32_t flags, char* out, int64_t cap, int64_t* out_off)
{
    if (!c) return CSV_E_INVALID;
    return alt_gather_run(c, n, pick, clip, flags, out, cap, out_off, nullptr);
}

int csv_name_support_join(csv_ctx* c, int64_t n_calls, const int64_t* support_off, const int64_t* support_sig, const int32_t* support_sig32, char* out, int64_t cap, int64_t* out_off)
{
    if (!c) return CSV_E_INVALID;
    return support_join_run(c, n_calls, support_off, support_sig, support_sig32, out, cap, out_off, nullptr);
}

}  // extern "C"
