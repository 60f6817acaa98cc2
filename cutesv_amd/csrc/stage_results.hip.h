// stage_results.hip.h — engine, device -> host: csv_batch_download (synchronous; settles an upload) and the pipelined delivery
// csv_batch_publish_async / csv_batch_publish_wait.  State: ResultState (the two result arenas, the publishes in flight, the
// landing zones), with the batch's host copies (BatchState h_seg / h_woff).  Host code only.
namespace {

constexpr int PUB_MAX_SPANS = 3;
struct PubLayout {                                   // the result arrays as the caller laid them out: runs of exactly adjacent arrays
    const char* host[15]; size_t bytes[15]; size_t stage_off[15];
    struct Span { const char* host; size_t bytes, stage_off; } span[15];
    int n_span = 0; size_t stage_bytes = 0;
};
void publish_spans(PubLayout& L)
{
    int idx[15], n = 0;
    for (int i = 0; i < 15; i++) if (L.host[i] && L.bytes[i]) idx[n++] = i;
    std::sort(idx, idx + n, [&](int x, int y) { return L.host[x] < L.host[y]; });
    L.n_span = 0; L.stage_bytes = 0;
    for (int q = 0; q < n; q++) {
        const int i = idx[q];
        if (L.n_span && L.span[L.n_span - 1].host + L.span[L.n_span - 1].bytes == L.host[i]) {
            auto& sp = L.span[L.n_span - 1];
            L.stage_off[i] = sp.stage_off + sp.bytes; sp.bytes += L.bytes[i];
        } else {
            // (a run starts at the same offset modulo 256 as on the host: every array keeps its alignment in the image)
            const size_t off = ((L.stage_bytes + 255) & ~(size_t)255) + ((uintptr_t)L.host[i] & 255);
            L.span[L.n_span++] = {L.host[i], L.bytes[i], off};
            L.stage_off[i] = off;
        }
        L.stage_bytes = L.span[L.n_span - 1].stage_off + L.span[L.n_span - 1].bytes;
    }
}
// Are all of the caller's call arrays page-locked (device addressable)?  Then fill `P` with their device addresses.
bool publish_targets(csv_ctx* c, const csv_batch_out* out, PublishArgs& P, PubLayout* L = nullptr, char* stage = nullptr)
{
    (void)c;
    if (c->opt.no_publish || out->cap_calls < 0 || out->cap_support < 0) return false;
    const size_t nc = (size_t)out->cap_calls, ns = (size_t)out->cap_support;
    const bool sup32 = out->support_sig32 != nullptr, nosup = (out->flags & CSV_OUT_NO_SUPPORT_LIST) != 0;
    const size_t cw = (out->flags & CSV_OUT_COORD_I32) ? 4 : 8;
    const void* host[15] = {out->call_seg, out->call_cluster, out->call_aux, out->support, out->cipos, out->cilen, out->dr, out->dv, out->gl_idx,
                            out->bp1, out->bp2, out->search_pos, out->seq_pick, out->support_off, sup32 ? (const void*)out->support_sig32 : (const void*)out->support_sig};
    const size_t bytes[15] = {nc * 4, nc * 4, nc * 4, nc * 4, nc * 4, nc * 4, nc * 4, nc * 4, nc * 4, nc * cw, nc * cw, nc * cw, nc * cw, (nc + 1) * 8, ns * (sup32 ? 4 : 8)};
    // (ABI v7) optional fields may be NULL: not written; every array that IS given must be page-locked
    const bool required[15] = {true, false, false, true, false, false, false, false, false, true, true, false, false, !nosup, !nosup};
    void* dev[15];
    for (int i = 0; i < 15; i++) {
        dev[i] = nullptr;
        if (nosup && i >= 13) continue;
        if (!host[i]) { if (required[i]) return false; continue; }
        if (stage) { dev[i] = stage + L->stage_off[i]; continue; }          // (second pass: the device image of a laid-out result)
        dev[i] = pinned_device_address(host[i], bytes[i] ? bytes[i] : 1);
        if (!dev[i]) return false;
    }
    if (L && !stage) {
        for (int i = 0; i < 15; i++) { L->host[i] = dev[i] ? (const char*)host[i] : nullptr; L->bytes[i] = dev[i] ? bytes[i] : 0; L->stage_off[i] = 0; }
        publish_spans(*L);
    }
    P.call_seg = (int*)dev[0]; P.call_cluster = (int*)dev[1]; P.call_aux = (int*)dev[2]; P.support = (int*)dev[3]; P.cipos = (int*)dev[4];
    P.cilen = (int*)dev[5]; P.dr = (int*)dev[6]; P.dv = (int*)dev[7]; P.gl_idx = (int*)dev[8];
    P.bp1 = dev[9]; P.bp2 = dev[10]; P.search_pos = dev[11]; P.seq_pick = dev[12]; P.support_off = (i64*)dev[13];
    P.support_sig = sup32 ? nullptr : (i64*)dev[14]; P.support_sig32 = sup32 ? (int*)dev[14] : nullptr;
    P.coord32 = cw == 4; P.no_support = nosup;
    return true;
}

// ---- pipelined delivery: the result of run k crosses PCIe while run k + 1 computes
int result_status(csv_ctx* c, const DevCounters& k, csv_batch_out* out, bool nosup)
{
    out->n_calls = k.n_calls; out->n_support = k.n_support; out->n_clusters = k.n_clusters;
    if (k.error & ERR_READS_UNSORTED) return fail(c, CSV_E_UNSORTED, "a reads block is not sorted by start although CSV_IN_READS_SORTED was set");
    if (k.error & ERR_CLUSTER_TOO_BIG) return fail(c, CSV_E_INVALID, "a chained cluster has more than %lld signatures", (long long)MAX_CLUSTER);
    if (k.error & ERR_KEY_RANGE) return fail(c, CSV_E_INVALID, "a read id is negative, or a read end is negative or >= 2^40");
    if (k.error & ERR_COVER_OVERFLOW) return fail(c, CSV_E_INVALID, "internal: the genotype hash pool was too small");
    if (k.error & ERR_TRA_CHROM) return fail(c, CSV_E_INVALID, "a TRA call names a mate chromosome outside the reads table");
    if (k.error & ERR_TMP_OVERFLOW) return fail(c, CSV_E_INVALID, "internal: temp call capacity exceeded");
    if (k.n_calls > out->cap_calls || (!nosup && k.n_support > out->cap_support))
        return fail(c, CSV_E_CAPACITY, "need %d calls / %lld supports", k.n_calls, (long long)k.n_support);
    return CSV_OK;
}

}  // namespace

extern "C" {

// Device -> host: the counters, then ONE copy of the call records and one of the support lists into the page-locked
// block, unpacked into the caller's arrays on the host (a few MB; the per-signature outputs only when they were asked
// for at upload).
int csv_batch_download(csv_ctx* c, csv_batch_out* out)
{
    if (!c || !out) return CSV_E_INVALID;
    if (!c->bt.ran) return fail(c, CSV_E_STATE, "csv_batch_download before csv_batch_run");
    if (c->res.n_pend) return fail(c, CSV_E_STATE, "csv_batch_download while %d asynchronous publish(es) are in flight: csv_batch_publish_wait first", c->res.n_pend);
    const bool nosup = (out->flags & CSV_OUT_NO_SUPPORT_LIST) != 0, coord32 = (out->flags & CSV_OUT_COORD_I32) != 0;
    if (!nosup && ((out->support_sig != nullptr) == (out->support_sig32 != nullptr) || !out->support_off))
        return fail(c, CSV_E_INVALID, "csv_batch_out: support_off and exactly one of support_sig / support_sig32 must be given (or CSV_OUT_NO_SUPPORT_LIST)");
    if (!out->call_seg || !out->bp1 || !out->bp2 || !out->support) return fail(c, CSV_E_INVALID, "csv_batch_out: call_seg, bp1, bp2 and support are required");
    if (coord32 && !c->bt.B.a.p32) return fail(c, CSV_E_INVALID, "CSV_OUT_COORD_I32 needs a batch of CSV_IN_SIG_I32 columns");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int S0 = (int)c->bt.h_seg.size();
    PublishArgs P{};
    bool published = false;
    if (publish_targets(c, out, P)) {
        // page-locked result arrays: k_publish writes everything in place; the download is one synchronisation
        const size_t o_cnt = 0, o_err = 256, need = o_err + (size_t)(S0 + 1) * 4;
        static_assert(sizeof(DevCounters) <= 256, "counters landing zone");
        if (need > c->h_pin_cap) { HIP_TRY(c, hipStreamSynchronize(st)); const int rc = pin_reserve(c, need); if (rc) return rc; }
        void* dpin = nullptr;
        HIP_TRY(c, hipHostGetDevicePointer(&dpin, c->h_pin, 0));
        P.cap_calls = out->cap_calls; P.cap_support = out->cap_support; P.n_seg = S0;
        P.h_cnt = (DevCounters*)((char*)dpin + o_cnt); P.h_seg_err = (int*)((char*)dpin + o_err);
        for (int attempt = 0; attempt < 2; attempt++) {
            hipLaunchKernelGGL(k_publish, dim3(512), dim3(256), 0, st, c->bt.B, P);
            HIP_TRY(c, hipStreamSynchronize(st));
            memcpy(&c->res.h_cnt, c->h_pin + o_cnt, sizeof(DevCounters));
            if (c->opt.debug_counters)
                fprintf(stderr, "[csv] counters (published): clusters %d items %d calls %d error %d | reads: mode %d runs %d state %d\n",
                        c->res.h_cnt.n_clusters, c->res.h_cnt.n_items, c->res.h_cnt.n_calls, c->res.h_cnt.error, c->bt.B.ro_mode, c->res.h_cnt.n_runs, c->res.h_cnt.ro_state);
            if (c->bt.B.ro_mode == 1 && c->bt.B.n_reads > 0 && c->bt.any_genotype && c->res.h_cnt.ro_state == RO_NEED_GENERAL && attempt == 0) {
                c->ro.reads_general = true;             // (as read_counters does: the batch again, through the general sort)
                c->bt.B.ro_mode = 2;
                c->ro.reads_ready = false;
                const int rc = run_impl(c, nullptr);
                if (rc) return rc;
                continue;
            }
            break;
        }
        published = true;
    } else {
        const int rc = read_counters(c);
        if (rc) return rc;
    }
    c->res.settled = true;
    const DevCounters& k = c->res.h_cnt;
    out->n_calls = k.n_calls; out->n_support = k.n_support; out->n_clusters = k.n_clusters;
    if (k.error & ERR_READS_UNSORTED) return fail(c, CSV_E_UNSORTED, "a reads block is not sorted by start although CSV_IN_READS_SORTED was set");
    if (k.error & ERR_CLUSTER_TOO_BIG) return fail(c, CSV_E_INVALID, "a chained cluster has more than %lld signatures", (long long)MAX_CLUSTER);
    if (k.error & ERR_KEY_RANGE) return fail(c, CSV_E_INVALID, "a read id is negative, or a read end is negative or >= 2^40");
    if (k.error & ERR_COVER_OVERFLOW) return fail(c, CSV_E_INVALID, "internal: the genotype hash pool was too small");
    if (k.error & ERR_TRA_CHROM) return fail(c, CSV_E_INVALID, "a TRA call names a mate chromosome outside the reads table");
    if (k.error & ERR_TMP_OVERFLOW) return fail(c, CSV_E_INVALID, "internal: temp call capacity exceeded");
    if ((out->cluster_id || out->allele_id) && !c->bt.B.per_sig)
        return fail(c, CSV_E_STATE, "cluster_id / allele_id requested but the batch was uploaded without CSV_IN_PER_SIG");
    if (k.n_calls > out->cap_calls || (!nosup && k.n_support > out->cap_support))
        return fail(c, CSV_E_CAPACITY, "need %d calls / %lld supports", k.n_calls, (long long)k.n_support);
    const size_t nc = (size_t)k.n_calls; size_t ns = (size_t)k.n_support;
    const DevBatch& B = c->bt.B;
    const int S = (int)c->bt.h_seg.size();
    const size_t o_rec = 256, o_err = published ? 256 : o_rec + ((nc * sizeof(CallRec) + 255) & ~(size_t)255), o_end = o_err + (size_t)(S + 1) * 4;
    int* sup_stage = nullptr;
    if (!published) {
    if (nosup) ns = 0;                                       // (the staging path below moves no support list then)
    if (o_end + (out->support_sig32 ? 0 : ns * 4) + 64 > c->h_pin_cap) { const int rc = pin_reserve(c, o_end + (out->support_sig32 ? 0 : ns * 4) + 64); if (rc) return rc; }
    // the call records first: they are unpacked on the host while the (larger) support list is still on its way
    if (nc) HIP_TRY(c, hipMemcpyAsync(c->h_pin + o_rec, B.o_rec, nc * sizeof(CallRec), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(c->ev_sel, st));
    // the support list is int32 on the device: straight into the caller's int32 array, or widened on the host behind the copy
    if (ns && out->support_sig32) HIP_TRY(c, hipMemcpyAsync(out->support_sig32, B.o_supsig, ns * 4, hipMemcpyDeviceToHost, st));
    else if (ns) { sup_stage = (int*)(c->h_pin + o_end); HIP_TRY(c, hipMemcpyAsync(sup_stage, B.o_supsig, ns * 4, hipMemcpyDeviceToHost, st)); }
    if (S) HIP_TRY(c, hipMemcpyAsync(c->h_pin + o_err, B.seg_err, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    }
    if (out->cluster_id) memset(out->cluster_id, 0xff, (size_t)c->bt.n_sig_host * 4);
    if (out->allele_id) memset(out->allele_id, 0xff, (size_t)c->bt.n_sig_host * 4);
    if (out->cluster_id || out->allele_id) {
        for (int s = 0; s < S;) {
            int e = s;
            while (e + 1 < S && c->bt.h_seg[e + 1].sig_begin == c->bt.h_seg[e].sig_end) e++;
            const i64 dst = c->bt.h_seg[s].sig_begin, n = c->bt.h_woff[e + 1] - c->bt.h_woff[s], src = c->bt.h_woff[s];
            if (n > 0 && out->cluster_id) HIP_TRY(c, hipMemcpyAsync(out->cluster_id + dst, B.cluster_id + src, n * 4, hipMemcpyDeviceToHost, st));
            if (n > 0 && out->allele_id) HIP_TRY(c, hipMemcpyAsync(out->allele_id + dst, B.allele_id + src, n * 4, hipMemcpyDeviceToHost, st));
            s = e + 1;
        }
    }
    if (!published) {
        HIP_TRY(c, hipEventSynchronize(c->ev_sel));
        const CallRec* r = (const CallRec*)(c->h_pin + o_rec);
        for (size_t i = 0; i < nc; i++) {
            const CallRec& x = r[i];
            out->call_seg[i] = x.seg; out->support[i] = x.support;
            if (out->call_cluster) out->call_cluster[i] = x.cluster;
            if (out->call_aux) out->call_aux[i] = x.aux;
            if (out->cipos) out->cipos[i] = x.cipos;
            if (out->cilen) out->cilen[i] = x.cilen;
            if (coord32) {
                ((int32_t*)out->bp1)[i] = (int32_t)x.bp1; ((int32_t*)out->bp2)[i] = (int32_t)x.bp2;
                if (out->search_pos) ((int32_t*)out->search_pos)[i] = (int32_t)x.search;
                if (out->seq_pick) ((int32_t*)out->seq_pick)[i] = (int32_t)x.pick;
            } else {
                out->bp1[i] = x.bp1; out->bp2[i] = x.bp2;
                if (out->search_pos) out->search_pos[i] = x.search;
                if (out->seq_pick) out->seq_pick[i] = x.pick;
            }
            if (out->dr) out->dr[i] = x.dr;
            if (out->dv) out->dv[i] = x.dv;
            if (out->gl_idx) out->gl_idx[i] = x.gl;
            if (!nosup) out->support_off[i] = x.supoff;
        }
        if (!nosup) out->support_off[nc] = (int64_t)ns;
    }
    if (!published || out->cluster_id || out->allele_id) HIP_TRY(c, hipStreamSynchronize(st));
    if (sup_stage) for (size_t i = 0; i < ns; i++) out->support_sig[i] = sup_stage[i];
    if (out->seg_status && S) memcpy(out->seg_status, c->h_pin + o_err, (size_t)S * 4);
    return CSV_OK;
}

int csv_batch_publish_async(csv_ctx* c, csv_batch_out* out)
{
    if (!c || !out) return CSV_E_INVALID;
    if (!c->bt.ran) return fail(c, CSV_E_STATE, "csv_batch_publish_async before csv_batch_run");
    if (!c->res.settled) return fail(c, CSV_E_STATE, "csv_batch_publish_async needs one csv_batch_download of this upload first (it settles how the reads table is ordered and what the result needs)");
    if (c->bt.B.per_sig || out->cluster_id || out->allele_id) return fail(c, CSV_E_INVALID, "csv_batch_publish_async delivers no per-signature outputs");
    if (c->res.pend[c->res.parity].live) return fail(c, CSV_E_STATE, "this run's result is already being published");
    if (c->res.n_pend >= 2) return fail(c, CSV_E_STATE, "two publishes in flight: csv_batch_publish_wait first");
    const bool nosup = (out->flags & CSV_OUT_NO_SUPPORT_LIST) != 0, coord32 = (out->flags & CSV_OUT_COORD_I32) != 0;
    if (!nosup && ((out->support_sig != nullptr) == (out->support_sig32 != nullptr) || !out->support_off))
        return fail(c, CSV_E_INVALID, "csv_batch_out: support_off and exactly one of support_sig / support_sig32 must be given (or CSV_OUT_NO_SUPPORT_LIST)");
    if (!out->call_seg || !out->bp1 || !out->bp2 || !out->support) return fail(c, CSV_E_INVALID, "csv_batch_out: call_seg, bp1, bp2 and support are required");
    if (coord32 && !c->bt.B.a.p32) return fail(c, CSV_E_INVALID, "CSV_OUT_COORD_I32 needs a batch of CSV_IN_SIG_I32 columns");
    HIP_TRY(c, hipSetDevice(c->device));
    PublishArgs P{};
    PubLayout L;
    if (!publish_targets(c, out, P, &L)) return fail(c, CSV_E_INVALID, "csv_batch_publish_async writes the result in place: every array of csv_batch_out must be page-locked (csv_host_alloc / csv_host_register)");
    const int S0 = (int)c->bt.h_seg.size(), p = c->res.parity;
    const size_t zone = (256 + (size_t)(S0 + 1) * 4 + 255) & ~(size_t)255;
    if (2 * zone > c->res.h_pub_cap) {
        if (c->res.n_pend) return fail(c, CSV_E_STATE, "internal: landing zones in use");
        if (c->res.h_pub) { HIP_TRY(c, hipHostFree(c->res.h_pub)); c->res.h_pub = nullptr; c->res.h_pub_cap = 0; }
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 2 * zone + 4096, hipHostMallocDefault) != hipSuccess) return fail(c, CSV_E_NOMEM, "hipHostMalloc for the publish landing zones failed");
        c->res.h_pub = (char*)hp; c->res.h_pub_cap = 2 * zone + 4096;
    }
    void* dpub = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&dpub, c->res.h_pub, 0));
    const size_t half = c->res.h_pub_cap / 2 & ~(size_t)255;
    // Block delivery (arrays back to back in page-locked memory: engine.result_buffers lays them out so).  A kernel that stores
    // across PCIe holds up every kernel BOUNDARY of the next run beside it - the end-of-kernel cache write-back waits for the
    // posted writes in flight, whoever issued them (measured: k_chain_apply 6 -> 62 us next to a k_publish of 3.4 MB, a step 110 us
    // = run + delivery, nothing overlapped) - while a copy-engine transfer leaves the kernels alone.  So: the image is written into
    // device memory behind the run's own kernels (main stream, ~4 us) and the copy engine moves it under the next run.
    const bool block = L.n_span > 0 && L.n_span <= PUB_MAX_SPANS && !c->opt.pub_inplace;
    if (block) {
        if (L.stage_bytes + 256 > c->res.pub_stage_cap[p]) {
            if (c->res.pub_stage[p]) { HIP_TRY(c, hipStreamSynchronize(c->res.pub)); HIP_TRY(c, hipFree(c->res.pub_stage[p])); c->res.pub_stage[p] = nullptr; c->res.pub_stage_cap[p] = 0; }
            const size_t cap = L.stage_bytes + L.stage_bytes / 8 + 4096;
            if (hipMalloc(&c->res.pub_stage[p], cap) != hipSuccess) return fail(c, CSV_E_NOMEM, "hipMalloc(%zu) for the result image failed", cap);
            c->res.pub_stage_cap[p] = cap;
        }
        if (!publish_targets(c, out, P, &L, (char*)c->res.pub_stage[p])) return fail(c, CSV_E_INVALID, "internal: result image");
    }
    P.cap_calls = out->cap_calls; P.cap_support = out->cap_support; P.n_seg = S0;
    P.h_cnt = (DevCounters*)((char*)dpub + half * p); P.h_seg_err = (int*)((char*)dpub + half * p + 256);
    const hipStream_t ps = c->res.pub;
    if (block) {
        hipLaunchKernelGGL(k_publish, dim3(512), dim3(256), 0, c->stream, c->bt.B, P);       // (c->bt.B points at arena p: the last run's)
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->res.ev_run[p], c->stream));
        HIP_TRY(c, hipStreamWaitEvent(ps, c->res.ev_run[p], 0));
        for (int q = 0; q < L.n_span; q++)
            HIP_TRY(c, hipMemcpyAsync((void*)L.span[q].host, (char*)c->res.pub_stage[p] + L.span[q].stage_off, L.span[q].bytes, hipMemcpyDeviceToHost, ps));
    } else {
        // (the run's kernels are all in the main stream's queue: an event recorded now marks their end - a plain run pays nothing for it)
        HIP_TRY(c, hipEventRecord(c->res.ev_run[p], c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->res.pub, c->res.ev_run[p], 0));
        hipLaunchKernelGGL(k_publish, dim3(512), dim3(256), 0, c->res.pub, c->bt.B, P);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->res.ev_pub[p], ps));
    c->res.pend[p].out = out; c->res.pend[p].live = true;
    c->res.pend_order[c->res.n_pend++] = p;
    return CSV_OK;
}

int csv_batch_publish_wait(csv_ctx* c, csv_batch_out** done)
{
    if (!c) return CSV_E_INVALID;
    if (done) *done = nullptr;
    if (!c->res.n_pend) return fail(c, CSV_E_STATE, "csv_batch_publish_wait: nothing in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    const int p = c->res.pend_order[0];
    HIP_TRY(c, hipEventSynchronize(c->res.ev_pub[p]));
    c->res.pend_order[0] = c->res.pend_order[1]; c->res.n_pend--;
    csv_batch_out* out = c->res.pend[p].out;
    c->res.pend[p].live = false; c->res.pend[p].out = nullptr;
    if (done) *done = out;
    const size_t half = c->res.h_pub_cap / 2 & ~(size_t)255;
    DevCounters k;
    memcpy(&k, c->res.h_pub + half * p, sizeof k);
    const int S = (int)c->bt.h_seg.size();
    if (out->seg_status && S) memcpy(out->seg_status, c->res.h_pub + half * p + 256, (size_t)S * 4);
    return result_status(c, k, out, (out->flags & CSV_OUT_NO_SUPPORT_LIST) != 0);
}

}  // extern "C"
