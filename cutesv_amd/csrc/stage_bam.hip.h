// stage_bam.hip.h — csv_bam_decode, csv_bam_split_inputs: a slim BAM chunk -> record columns and CIGAR operations, its SA tags -> the
// entry columns of the split-read analysis (BamState / SaState in ctx.hip.h; bam.hip.h, sa.hip.h).  Host code; included by cutesv_hip.hip.
extern "C" {

// csv_bam_decode; with dev_slim (csv_bam_decode_framed, stage_frame.hip.h) the slim image lies in device memory already and is copied
// there: what crosses the link is rec_off and rec_len alone
static int bam_decode_impl(csv_ctx* c, const csv_bam_in* in, csv_bam_out* out, const uint8_t* dev_slim)
{
    if (!c || !in || !out) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    out->n_ops = out->n_sa = out->n_bad = out->bytes_uploaded = 0; out->ms_device = out->ms_upload = 0;
    out->dev_ref_start = out->dev_ref_end = out->dev_flag = out->dev_mapq = out->dev_query_len = out->dev_clip_left = out->dev_clip_right =
        out->dev_cls = out->dev_cig_off = out->dev_cigar = nullptr;
    c->bm.n = -1; c->bm.gates_ok = false; c->sa.calls = -1; c->seq.n_reads = -1; c->seq.n_qrev = -1;      // (the uploaded read sequences belong to the previous batch)
    const i64 n = in->n_records, nb = in->slim_bytes;
    if (n < 0 || nb < 0 || in->flags != 0 || (n > 0 && ((!in->slim && !dev_slim) || !in->rec_off || !in->rec_len))) return fail(c, CSV_E_INVALID, "bad BAM chunk header");
    if (n >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "BAM chunk too large (%lld records): split it", (long long)n);
    // the kernels read [rec_off, rec_off + rec_len) of every record and nothing else: each range is checked against the image
    for (i64 r = 0; r < n; r++) {
        const i64 o = in->rec_off[r], l = in->rec_len[r];
        if (o < 0 || (o & 15) || l < 32 || o > nb || l > nb - o) return fail(c, CSV_E_INVALID, "record %lld of the BAM chunk leaves the slim image (or is misaligned / shorter than 32 bytes)", (long long)r);
    }
    if (n == 0) { c->bm.n = 0; c->bm.nops = 0; c->bm.nsa = 0; if (out->cig_off) out->cig_off[0] = 0; if (out->sa_off) out->sa_off[0] = 0; return CSV_OK; }
    const i64 max_ops = nb / 4;                              // every operation is 4 bytes of the image
    Plan P;
    P.add(c->bm.slim, nb + 16); P.add(c->bm.recoff, n * 8); P.add(c->bm.reclen, n * 4);
    P.add(c->bm.start, n * 8); P.add(c->bm.end, n * 8); P.add(c->bm.flag, n * 4); P.add(c->bm.mapq, n * 4); P.add(c->bm.qlen, n * 4); P.add(c->bm.cl, n * 4); P.add(c->bm.cr, n * 4);
    P.add(c->bm.cls, n); P.add(c->bm.status, n); P.add(c->bm.cigoff, (n + 1) * 8); P.add(c->bm.saoff, (n + 1) * 8); P.add(c->bm.cigsrc, n * 8); P.add(c->bm.cgb, n * 8); P.add(c->bm.cge, n * 8);
    P.add(c->bm.cigar, (max_ops + 1) * 4); P.add(c->bm.long_list, n * 4); P.add(c->bm.cnt, 16); P.add(c->bm.tot, 16);
    TRY(commit_synced(c, c->bm.arena, P));
    hipStream_t st = c->stream;
    HIP_TRY(c, hipEventRecord(c->ev[4], st));
    if (dev_slim) { if (nb > 0) HIP_TRY(c, hipMemcpyAsync(c->bm.slim.p, dev_slim, (size_t)nb, hipMemcpyDeviceToDevice, st)); }
    else TRY(h2d(c, c->bm.slim, in->slim, nb));
    TRY(h2d(c, c->bm.recoff, in->rec_off, n * 8)); TRY(h2d(c, c->bm.reclen, in->rec_len, n * 4));
    HIP_TRY(c, hipEventRecord(c->ev[5], st));
    out->bytes_uploaded = (dev_slim ? 0 : nb) + n * 12;
    HIP_TRY(c, hipMemsetAsync(c->bm.cnt.p, 0, 16, st));
    BamArgs A{};
    A.n = n; A.slim = dp<uint8_t>(c->bm.slim); A.rec_off = dp<i64>(c->bm.recoff); A.rec_len = dp<unsigned>(c->bm.reclen);
    A.ref_start = dp<i64>(c->bm.start); A.ref_end = dp<i64>(c->bm.end); A.flag = dp<int>(c->bm.flag); A.mapq = dp<int>(c->bm.mapq); A.qlen = dp<int>(c->bm.qlen);
    A.clip_l = dp<int>(c->bm.cl); A.clip_r = dp<int>(c->bm.cr); A.cls = dp<uint8_t>(c->bm.cls); A.status = dp<uint8_t>(c->bm.status);
    A.cig_off = dp<i64>(c->bm.cigoff); A.sa_off = dp<i64>(c->bm.saoff); A.cig_src = dp<i64>(c->bm.cigsrc); A.cg_beg = dp<i64>(c->bm.cgb); A.cg_end = dp<i64>(c->bm.cge);
    A.cigar = dp<unsigned>(c->bm.cigar); A.long_list = dp<int>(c->bm.long_list); A.counters = dp<int>(c->bm.cnt); A.totals = dp<i64>(c->bm.tot);
    TwoPhaseTimer T{c};
    TRY(T.count_begin());
    hipLaunchKernelGGL(k_bam_fixed, dim3(div_up(n, 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, A);
    TRY(T.count_end());
    i64 tot[2] = {0, 0};
    int cnt[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(tot, c->bm.tot.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(cnt, c->bm.cnt.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    // (what the kernels counted is bounded by the image they counted it in; anything else would be a bug here, not in the file)
    if (tot[0] < 0 || tot[0] > max_ops || tot[1] < 0 || tot[1] > nb / 4 || cnt[0] < 0 || cnt[0] > n)
        return fail(c, CSV_E_INVALID, "BAM decode: inconsistent counts (%lld operations, %lld SA tags)", (long long)tot[0], (long long)tot[1]);
    out->n_ops = tot[0]; out->n_sa = tot[1]; out->n_bad = cnt[1];
    if ((out->cigar && tot[0] > out->cap_ops) || ((out->sa_beg || out->sa_end) && tot[1] > out->cap_sa))
        return fail(c, CSV_E_CAPACITY, "need %lld CIGAR operations / %lld SA ranges", (long long)tot[0], (long long)tot[1]);
    TRY(reserve(c, c->bm.sabeg, (size_t)(tot[1] + 1) * 8)); TRY(reserve(c, c->bm.saend, (size_t)(tot[1] + 1) * 8));
    A.sa_beg = dp<i64>(c->bm.sabeg); A.sa_end = dp<i64>(c->bm.saend);
    TRY(T.emit_begin());
    const int grid = div_up(n, 4) < 8192 ? div_up(n, 4) : 8192;
    hipLaunchKernelGGL(k_bam_cigar, dim3(grid), dim3(256), 0, st, A);
    if (cnt[0] > 0) hipLaunchKernelGGL(k_bam_cigar_long, dim3(cnt[0]), dim3(256), 0, st, A);
    if (tot[1] > 0) hipLaunchKernelGGL(k_bam_sa, dim3(div_up(n, 256)), dim3(256), 0, st, A);
    TRY(T.emit_end());
    // (an output array that is NULL is not written)
    const HostCol cols[] = {{out->ref_start, &c->bm.start, n * 8}, {out->ref_end, &c->bm.end, n * 8}, {out->flag, &c->bm.flag, n * 4}, {out->mapq, &c->bm.mapq, n * 4},
                            {out->query_len, &c->bm.qlen, n * 4}, {out->clip_left, &c->bm.cl, n * 4}, {out->clip_right, &c->bm.cr, n * 4}, {out->cls, &c->bm.cls, n},
                            {out->status, &c->bm.status, n}, {out->cig_off, &c->bm.cigoff, (n + 1) * 8}, {out->cigar, &c->bm.cigar, tot[0] * 4},
                            {out->sa_off, &c->bm.saoff, (n + 1) * 8}, {out->sa_beg, &c->bm.sabeg, tot[1] * 8}, {out->sa_end, &c->bm.saend, tot[1] * 8},
                            {out->cg_beg, &c->bm.cgb, n * 8}, {out->cg_end, &c->bm.cge, n * 8}};
    for (const HostCol& o : cols) TRY(d2h(c, o.host, *o.dev, o.bytes, false));
    HIP_TRY(c, hipStreamSynchronize(st));
    TRY(T.elapsed(&out->ms_device));
    HIP_TRY(c, hipEventElapsedTime(&out->ms_upload, c->ev[4], c->ev[5]));
    if (cnt[1] > 0) return fail(c, CSV_E_INVALID, "%d record(s) of the BAM chunk have a malformed aux area or CIGAR (see status)", cnt[1]);
    out->dev_ref_start = c->bm.start.p; out->dev_ref_end = c->bm.end.p; out->dev_flag = c->bm.flag.p; out->dev_mapq = c->bm.mapq.p; out->dev_query_len = c->bm.qlen.p;
    out->dev_clip_left = c->bm.cl.p; out->dev_clip_right = c->bm.cr.p; out->dev_cls = c->bm.cls.p; out->dev_cig_off = c->bm.cigoff.p; out->dev_cigar = c->bm.cigar.p;
    c->bm.n = n; c->bm.nops = tot[0]; c->bm.nsa = tot[1];
    return CSV_OK;
}

int csv_bam_decode(csv_ctx* c, const csv_bam_in* in, csv_bam_out* out) { return bam_decode_impl(c, in, out, nullptr); }

int csv_sa_struct_size(int which) { return which == 0 ? (int)sizeof(csv_sa_in) : which == 1 ? (int)sizeof(csv_sa_out) : -1; }

int csv_bam_split_inputs(csv_ctx* c, const csv_sa_in* in, csv_sa_out* out)
{
    if (!c || !in || !out) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    out->n_calls = out->n_entries = out->n_flagged = 0; out->ms_device = 0;
    c->sa.calls = -1;
    const i64 n = in->n_records, nn = in->n_names, nbytes = in->name_bytes;
    if (c->bm.n < 0) return fail(c, CSV_E_INVALID, "csv_bam_split_inputs: the context holds no decoded BAM chunk");
    if (n != c->bm.n) return fail(c, CSV_E_INVALID, "csv_bam_split_inputs: n_records is not the record count of the context's last csv_bam_decode");
    // CSV_SA_SEL_FROM_GATES: sel[i] is the CSV_GATE_SEL bit of the column csv_bam_task_gates left beside the decode
    const bool sel_gates = (in->flags & CSV_SA_SEL_FROM_GATES) != 0;
    if (sel_gates && (in->sel || !c->bm.gates_ok))
        return fail(c, CSV_E_INVALID, "CSV_SA_SEL_FROM_GATES needs sel = NULL and the gates of the context's last csv_bam_decode (csv_bam_task_gates)");
    if ((in->flags & ~CSV_SA_SEL_FROM_GATES) != 0 || nn < 0 || nbytes < 0 || (n > 0 && !in->sel && !sel_gates) || (nn > 0 && (!in->name_off || !in->name_rank)) || (nbytes > 0 && !in->names))
        return fail(c, CSV_E_INVALID, "bad split-input header");
    // the kernels index `names` with these offsets and search the table by halving: both are checked here
    for (i64 k = 0; k < nn; k++) {
        const i64 b = in->name_off[k], e = in->name_off[k + 1];
        if (b < 0 || e < b || e > nbytes) return fail(c, CSV_E_INVALID, "name_off decreases or leaves the name bytes at name %lld", (long long)k);
        if (k > 0) {
            const i64 pb = in->name_off[k - 1], pl = b - pb, l = e - b;
            int cmp = memcmp(in->names + pb, in->names + b, (size_t)(pl < l ? pl : l));
            if (cmp == 0) cmp = pl < l ? -1 : pl > l ? 1 : 0;
            if (cmp >= 0) return fail(c, CSV_E_INVALID, "the contig names are not strictly ascending in byte order at name %lld", (long long)k);
        }
    }
    const i64 max_calls = c->bm.nsa;                        // every call is an SA tag of the chunk
    if (n == 0 || max_calls == 0) {
        if (out->ent_off) out->ent_off[0] = 0;
        c->sa.calls = 0; c->sa.entries = 0;
        return CSV_OK;
    }
    Plan P;
    P.add(c->sa.sel, n); P.add(c->sa.names, nbytes + 1); P.add(c->sa.nameoff, (nn + 1) * 8); P.add(c->sa.namerank, (nn + 1) * 4);
    P.add(c->sa.calloff, (n + 1) * 8); P.add(c->sa.callrec, (max_calls + 1) * 4); P.add(c->sa.callsa, (max_calls + 1) * 8); P.add(c->sa.entoff, (max_calls + 1) * 8);
    P.add(c->sa.readlen, (max_calls + 1) * 8); P.add(c->sa.status, max_calls + 1); P.add(c->sa.tot, 32);
    TRY(commit_synced(c, c->sa.arena, P));
    hipStream_t st = c->stream;
    if (!sel_gates) TRY(h2d(c, c->sa.sel, in->sel, n));
    TRY(h2d(c, c->sa.names, in->names, nbytes));
    if (nn) { TRY(h2d(c, c->sa.nameoff, in->name_off, (nn + 1) * 8)); TRY(h2d(c, c->sa.namerank, in->name_rank, nn * 4)); }
    HIP_TRY(c, hipMemsetAsync(c->sa.tot.p, 0, 32, st));
    SaArgs A{};
    A.n = n; A.cap_calls = max_calls; A.cap_entries = 0;
    A.slim = dp<uint8_t>(c->bm.slim); A.sa_off = dp<i64>(c->bm.saoff); A.sa_beg = dp<i64>(c->bm.sabeg); A.sa_end = dp<i64>(c->bm.saend);
    A.flag = dp<int>(c->bm.flag); A.mapq = dp<int>(c->bm.mapq); A.qlen = dp<int>(c->bm.qlen); A.clip_l = dp<int>(c->bm.cl); A.clip_r = dp<int>(c->bm.cr);
    A.ref_start = dp<i64>(c->bm.start); A.ref_end = dp<i64>(c->bm.end);
    A.sel = sel_gates ? dp<uint8_t>(c->bm.gates) : dp<uint8_t>(c->sa.sel); A.sel_mask = sel_gates ? CSV_GATE_SEL : 255; A.min_mapq = in->min_mapq; A.task_rank = in->task_rank;
    A.names = dp<uint8_t>(c->sa.names); A.name_off = dp<i64>(c->sa.nameoff); A.name_rank = dp<int>(c->sa.namerank); A.n_names = (int)nn;
    A.call_off = dp<i64>(c->sa.calloff); A.call_rec = dp<int>(c->sa.callrec); A.call_sa = dp<i64>(c->sa.callsa); A.ent_off = dp<i64>(c->sa.entoff);
    A.read_len = dp<i64>(c->sa.readlen); A.status = dp<uint8_t>(c->sa.status); A.tot = dp<i64>(c->sa.tot);
    TwoPhaseTimer T{c};
    TRY(T.count_begin());
    hipLaunchKernelGGL(k_sa_mark, dim3(div_up(n, 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_sa_scan, dim3(1), dim3(1024), 0, st, A.call_off, n, (const i64*)nullptr, n, A.tot);
    hipLaunchKernelGGL(k_sa_calls, dim3(div_up(n, 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_sa_parse<false>, dim3(max_calls < 8192 ? (int)max_calls : 8192), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_sa_scan, dim3(1), dim3(1024), 0, st, A.ent_off, (i64)0, (const i64*)A.tot, max_calls, A.tot + 1);
    TRY(T.count_end());
    i64 tot[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(tot, c->sa.tot.p, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    // (what the kernels counted is bounded by the text they counted it in; anything else would be a bug here, not in the file)
    if (tot[0] < 0 || tot[0] > max_calls || tot[1] < 0 || tot[1] > c->bm.slim.cap + max_calls || tot[2] < 0 || tot[2] > tot[0])
        return fail(c, CSV_E_INVALID, "split inputs: inconsistent counts (%lld calls, %lld entries)", (long long)tot[0], (long long)tot[1]);
    const i64 nc = tot[0], ne = tot[1];
    out->n_calls = nc; out->n_entries = ne; out->n_flagged = tot[2];
    TRY(T.elapsed(&out->ms_device));          // (the count phase alone: what a capacity error reports)
    const bool want_calls = out->ent_off || out->read_len || out->call_rec || out->status;
    const bool want_entries = out->c0 || out->c1 || out->f0 || out->f1 || out->chr || out->mapq || out->strand || out->primary;
    if ((want_calls && nc > out->cap_calls) || (want_entries && ne > out->cap_entries))
        return fail(c, CSV_E_CAPACITY, "need %lld calls / %lld entries", (long long)nc, (long long)ne);
    Buf* ent[8] = {&c->sa.c0, &c->sa.c1, &c->sa.f0, &c->sa.f1, &c->sa.chr, &c->sa.mapq, &c->sa.strand, &c->sa.primary};
    const size_t ent_w[8] = {8, 8, 8, 8, 4, 4, 1, 1};
    for (int k = 0; k < 8; k++) TRY(reserve(c, *ent[k], (size_t)(ne + 1) * ent_w[k]));
    A.cap_entries = ne;
    A.c0 = dp<i64>(c->sa.c0); A.c1 = dp<i64>(c->sa.c1); A.f0 = dp<i64>(c->sa.f0); A.f1 = dp<i64>(c->sa.f1);
    A.chr = dp<int>(c->sa.chr); A.emapq = dp<int>(c->sa.mapq); A.strand = dp<uint8_t>(c->sa.strand); A.primary = dp<uint8_t>(c->sa.primary);
    if (nc > 0 && ne > 0) {
        TRY(T.emit_begin());
        hipLaunchKernelGGL(k_sa_parse<true>, dim3(nc < 8192 ? (int)nc : 8192), dim3(64), 0, st, A);
        TRY(T.emit_end());
    }
    // (an output array that is NULL is not written)
    const HostCol cols[] = {{out->ent_off, &c->sa.entoff, (nc + 1) * 8}, {out->read_len, &c->sa.readlen, nc * 8}, {out->call_rec, &c->sa.callrec, nc * 4}, {out->status, &c->sa.status, nc},
                            {out->c0, &c->sa.c0, ne * 8}, {out->c1, &c->sa.c1, ne * 8}, {out->f0, &c->sa.f0, ne * 8}, {out->f1, &c->sa.f1, ne * 8},
                            {out->chr, &c->sa.chr, ne * 4}, {out->mapq, &c->sa.mapq, ne * 4}, {out->strand, &c->sa.strand, ne}, {out->primary, &c->sa.primary, ne}};
    for (const HostCol& o : cols) TRY(d2h(c, o.host, *o.dev, o.bytes, false));
    HIP_TRY(c, hipStreamSynchronize(st));
    TRY(T.elapsed(&out->ms_device));
    c->sa.calls = nc; c->sa.entries = ne;
    return CSV_OK;
}

}  // extern "C"
