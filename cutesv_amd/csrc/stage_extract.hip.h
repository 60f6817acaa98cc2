// stage_extract.hip.h — csv_cigar_signatures, csv_split_signatures: the two extraction scans, each a count phase, the totals back for the
// capacity check, an emit phase (CigarState / SplitState in ctx.hip.h; cigar.hip.h, split.hip.h).  Host code; included by cutesv_hip.hip.
extern "C" {

int csv_cigar_signatures(csv_ctx* c, const csv_cigar_in* in, csv_cigar_out* out)
{
    if (!c || !in || !out) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    out->n_sig_ins = out->n_piece_ins = out->n_sig_del = 0; out->ms_device = 0;
    const i64 n = in->n_reads;
    // CSV_CG_FROM_BAM: the columns are the ones csv_bam_decode left on the device (offsets from its own scan: they start at 0,
    // do not decrease and end at its operation count)
    const bool from_bam = (in->flags & CSV_CG_FROM_BAM) != 0;
    if (from_bam && (c->bm.n < 0 || n != c->bm.n)) return fail(c, CSV_E_INVALID, "CSV_CG_FROM_BAM: n_reads is not the record count of the context's last csv_bam_decode");
    if (n < 0 || (n > 0 && !from_bam && (!in->cig_off || !in->ref_start))) return fail(c, CSV_E_INVALID, "bad CIGAR batch header");
    // CSV_CG_USE_FROM_GATES: use[r] is the CSV_GATE_USE bit of the column csv_bam_task_gates left beside that decode
    const bool use_gates = (in->flags & CSV_CG_USE_FROM_GATES) != 0;
    if (use_gates && (!from_bam || in->use || !c->bm.gates_ok))
        return fail(c, CSV_E_INVALID, "CSV_CG_USE_FROM_GATES needs CSV_CG_FROM_BAM, use = NULL and the gates of the context's last csv_bam_decode (csv_bam_task_gates)");
    // CSV_CG_SEQ_TO_POOL: the INS rows' bases are cut out of the uploaded read sequences, whose index space is this batch's
    const bool seq_to_pool = (in->flags & CSV_CG_SEQ_TO_POOL) != 0;
    if (seq_to_pool && !(in->flags & CSV_CG_TO_POOL)) return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL needs CSV_CG_TO_POOL");
    if (seq_to_pool && c->seq.n_reads != n) return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL: the context holds no read sequences for this batch (csv_seq_reads_upload with n_reads = %lld)", (long long)n);
    if (n == 0) return CSV_OK;
    const i64 nops = from_bam ? c->bm.nops : in->cig_off[n] - in->cig_off[0];
    if (!from_bam && (in->cig_off[0] != 0 || nops < 0 || (nops > 0 && !in->cigar))) return fail(c, CSV_E_INVALID, "cig_off must start at 0 and not decrease");
    if (nops >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "CIGAR batch too large (%lld operations): split it", (long long)nops);
    for (i64 r = 0; r < n && !from_bam; r++)                    // the kernels index `cigar` with these: every offset is checked here
        if (in->cig_off[r] < 0 || in->cig_off[r + 1] < in->cig_off[r] || in->cig_off[r + 1] > nops)
            return fail(c, CSV_E_INVALID, "cig_off decreases or leaves the CIGAR array at read %lld", (long long)r);
    // every op can be a piece and a signature of its own: size the outputs for the worst case the caller allows, but never
    // more than the operations there are
    const i64 cap_i = out->cap_sig_ins < nops ? out->cap_sig_ins : nops, cap_p = out->cap_piece_ins < nops ? out->cap_piece_ins : nops,
              cap_d = out->cap_sig_del < nops ? out->cap_sig_del : nops;
    Plan P;
    const bool to_pool = (in->flags & CSV_CG_TO_POOL) != 0;
    if (!from_bam) { P.add(c->cg.off, (n + 1) * 8); P.add(c->cg.ops, (nops + 1) * 4); P.add(c->cg.start, n * 8); }
    P.add(c->cg.use, n); P.add(c->cg.cnt, n * 16);
    if (to_pool && in->query_len) P.add(c->cg.qlen, n * 4);
    P.add(c->cg.tiles, scan_tile_bytes(n)); P.add(c->cg.tot, 32);
    P.add(c->cg.iread, (cap_i + 1) * 4); P.add(c->cg.ipos, (cap_i + 1) * 8); P.add(c->cg.ilen, (cap_i + 1) * 8); P.add(c->cg.ip0, (cap_i + 1) * 8); P.add(c->cg.inp, (cap_i + 1) * 4);
    P.add(c->cg.pq, (cap_p + 1) * 4); P.add(c->cg.pl, (cap_p + 1) * 4);
    P.add(c->cg.dread, (cap_d + 1) * 4); P.add(c->cg.dpos, (cap_d + 1) * 8); P.add(c->cg.dlen, (cap_d + 1) * 8);
    c->vs.stale();                                          // (the scratch arena is planned afresh: a kept rebuild's columns are gone)
    TRY(commit_synced(c, c->scratch, P));
    hipStream_t st = c->stream;
    if (!from_bam) { TRY(h2d(c, c->cg.off, in->cig_off, (n + 1) * 8)); TRY(h2d(c, c->cg.ops, in->cigar, nops * 4)); TRY(h2d(c, c->cg.start, in->ref_start, n * 8)); }
    if (in->use) TRY(h2d(c, c->cg.use, in->use, n));
    CigarArgs A{};
    A.n_reads = n; A.cig_off = dp<i64>(c->cg.off); A.cigar = dp<unsigned>(c->cg.ops); A.ref_start = dp<i64>(c->cg.start);
    if (from_bam) { A.cig_off = dp<i64>(c->bm.cigoff); A.cigar = dp<unsigned>(c->bm.cigar); A.ref_start = dp<i64>(c->bm.start); }
    A.use = in->use ? dp<uint8_t>(c->cg.use) : use_gates ? dp<uint8_t>(c->bm.gates) : nullptr;
    A.use_mask = use_gates ? CSV_GATE_USE : 255;
    A.min_siglength = in->min_siglength; A.merge_ins = in->merge_ins_threshold; A.merge_del = in->merge_del_threshold;
    A.cnt = dp<int4>(c->cg.cnt);
    A.ins_read = dp<int>(c->cg.iread); A.ins_pos = dp<i64>(c->cg.ipos); A.ins_len = dp<i64>(c->cg.ilen); A.ins_piece0 = dp<i64>(c->cg.ip0);
    A.ins_npiece = dp<int>(c->cg.inp); A.piece_qoff = dp<int>(c->cg.pq); A.piece_len = dp<int>(c->cg.pl);
    A.del_read = dp<int>(c->cg.dread); A.del_pos = dp<i64>(c->cg.dpos); A.del_len = dp<i64>(c->cg.dlen);
    const int grid = div_up(n, 4) < 4096 ? div_up(n, 4) : 4096;
    TwoPhaseTimer T{c};
    TRY(T.count_begin());
    hipLaunchKernelGGL(k_cigar_count, dim3(grid), dim3(256), 0, st, A);
    scan_counts(st, ScanArgs{n, A.cnt, dp<i64>(c->cg.tiles), dp<i64>(c->cg.tot)});
    TRY(T.count_end());
    i64 tot[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(tot, c->cg.tot.p, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    out->n_sig_ins = tot[0]; out->n_piece_ins = tot[1]; out->n_sig_del = tot[2];
    if (tot[0] > out->cap_sig_ins || tot[1] > out->cap_piece_ins || tot[2] > out->cap_sig_del)
        return fail(c, CSV_E_CAPACITY, "need %lld INS signatures / %lld INS pieces / %lld DEL signatures", (long long)tot[0], (long long)tot[1], (long long)tot[2]);
    TRY(T.emit_begin());
    hipLaunchKernelGGL(k_cigar_emit, dim3(grid), dim3(256), 0, st, A);
    TRY(T.emit_end());
    if (to_pool && tot[0] + tot[2] > 0) {
        PoolCols PC;
        TRY(pool_attach(c, in->read_base, n, tot[0] + tot[2], &PC));
        if (in->query_len) TRY(h2d(c, c->cg.qlen, in->query_len, n * 4));
        hipLaunchKernelGGL(k_pool_from_cigar, dim3(div_up(tot[0] + tot[2], 256)), dim3(256), 0, st, PC, c->pool.n, A, tot[0], tot[2], in->seg_ins, in->seg_del,
                           in->read_base, in->query_len ? dp<int>(c->cg.qlen) : seq_to_pool ? dp<int>(c->seq.rlen) : nullptr);
        HIP_TRY(c, hipGetLastError());
        if (seq_to_pool) {
            const SeqReads SR{dp<uint8_t>(c->seq.rbytes), dp<i64>(c->seq.roff), dp<int>(c->seq.rlen), c->seq.n_reads};
            const i64 base = c->pool.n;
            TRY(seq_attach(c, tot[0] + tot[2], tot[0],
                           [&](int4* cnt, int* err) { hipLaunchKernelGGL(k_seq_plan_cigar, dim3(div_up(tot[0], 256)), dim3(256), 0, st, SR, A, tot[0], dp<int>(c->pool.aux) + base, cnt, err); },
                           [&](const int4* cnt, SeqPool SP, i64 blob_base) { hipLaunchKernelGGL(k_seq_gather_cigar, dim3(div_up(tot[0], 4)), dim3(256), 0, st, SR, SP, A, tot[0], cnt, base, blob_base); }));
        }
        c->pool.n += tot[0] + tot[2];
    }
    // (with CSV_CG_TO_POOL an output array that is NULL is not written)
    const HostCol cols[] = {{out->ins_read, &c->cg.iread, tot[0] * 4}, {out->ins_pos, &c->cg.ipos, tot[0] * 8}, {out->ins_len, &c->cg.ilen, tot[0] * 8},
                            {out->ins_piece0, &c->cg.ip0, tot[0] * 8}, {out->ins_npiece, &c->cg.inp, tot[0] * 4},
                            {out->piece_qoff, &c->cg.pq, tot[1] * 4}, {out->piece_len, &c->cg.pl, tot[1] * 4},
                            {out->del_read, &c->cg.dread, tot[2] * 4}, {out->del_pos, &c->cg.dpos, tot[2] * 8}, {out->del_len, &c->cg.dlen, tot[2] * 8}};
    for (const HostCol& o : cols) TRY(d2h(c, o.host, *o.dev, o.bytes, !to_pool));
    HIP_TRY(c, hipStreamSynchronize(st));
    TRY(T.elapsed(&out->ms_device));
    return CSV_OK;
}

int csv_split_signatures(csv_ctx* c, const csv_split_in* in, csv_split_out* out)
{
    if (!c || !in || !out) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    out->n = 0; out->ms_device = 0;
    // CSV_SP_FROM_BAM: the reads are the calls csv_bam_split_inputs left on the device, with its entry columns (offsets from
    // its own scan: they start at 0, do not decrease and end at its entry count)
    const bool from_bam = (in->flags & CSV_SP_FROM_BAM) != 0;
    if (from_bam && (c->sa.calls < 0 || c->bm.n < 0)) return fail(c, CSV_E_INVALID, "CSV_SP_FROM_BAM: the context holds no split inputs (csv_bam_split_inputs after the last csv_bam_decode)");
    const i64 n = from_bam ? c->sa.calls : in->n_reads;
    if (n < 0 || (n > 0 && !from_bam && (!in->ent_off || !in->read_len))) return fail(c, CSV_E_INVALID, "bad split-read batch header");
    const bool seq_to_pool = (in->flags & CSV_CG_SEQ_TO_POOL) != 0;
    if (seq_to_pool && !(in->flags & CSV_CG_TO_POOL)) return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL needs CSV_CG_TO_POOL");
    if (seq_to_pool && c->seq.n_reads != (from_bam ? c->bm.n : n))
        return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL: the context holds no read sequences for this batch (csv_seq_reads_upload with n_reads = %lld)", (long long)(from_bam ? c->bm.n : n));
    if (seq_to_pool && !from_bam && c->seq.n_qrev != n) return fail(c, CSV_E_INVALID, "CSV_CG_SEQ_TO_POOL: the reads' strands are missing (csv_seq_query_reverse)");
    if (n == 0) return CSV_OK;
    const i64 ne = from_bam ? c->sa.entries : in->ent_off[n] - in->ent_off[0];
    if (!from_bam) {
        if (in->ent_off[0] != 0 || ne < 0) return fail(c, CSV_E_INVALID, "ent_off must start at 0 and not decrease");
        if (ne > 0 && (!in->c0 || !in->c1 || !in->f0 || !in->f1 || !in->chr || !in->mapq || !in->strand || !in->primary))
            return fail(c, CSV_E_INVALID, "split-read entry columns missing");
    }
    if (ne >= (1ll << 31) - 4096 || n >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "split-read batch too large: split it");
    for (i64 r = 0; r < n && !from_bam; r++)
        if (in->ent_off[r + 1] < in->ent_off[r]) return fail(c, CSV_E_INVALID, "ent_off decreases at read %lld", (long long)r);
    // the candidate columns are sized for what the caller allows, but never for more than the entries can yield: a read of s
    // segments emits nothing for s < 2, at most 3 candidates for s = 2 and at most 12 per window of three plus 2 for s >= 3
    // (split_read: the rules of one window that can fire together put 2 + 2 + 6 + 2) - at most 12 per entry either way
    const i64 cap_max = 12 * ne, cap = out->cap < 0 ? 0 : out->cap < cap_max ? out->cap : cap_max;
    Plan P;
    if (!from_bam) {
        P.add(c->sp.off, (n + 1) * 8); P.add(c->sp.len, n * 8); P.add(c->sp.c0, (ne + 1) * 8); P.add(c->sp.c1, (ne + 1) * 8); P.add(c->sp.f0, (ne + 1) * 8); P.add(c->sp.f1, (ne + 1) * 8);
        P.add(c->sp.chr, (ne + 1) * 4); P.add(c->sp.mapq, (ne + 1) * 4); P.add(c->sp.strand, ne + 1); P.add(c->sp.primary, ne + 1);
    }
    P.add(c->sp.seg, (ne + 1) * sizeof(SpSeg));
    P.add(c->sp.cnt, n * 16); P.add(c->sp.tiles, scan_tile_bytes(n)); P.add(c->sp.tot, 32);
    P.add(c->sp.kind, cap + 1); P.add(c->sp.read, (cap + 1) * 4); P.add(c->sp.ochr, (cap + 1) * 4); P.add(c->sp.aux, (cap + 1) * 4);
    P.add(c->sp.a, (cap + 1) * 8); P.add(c->sp.b, (cap + 1) * 8); P.add(c->sp.c, (cap + 1) * 8); P.add(c->sp.d, (cap + 1) * 8);
    c->vs.stale();                                          // (the scratch arena is planned afresh: a kept rebuild's columns are gone)
    TRY(commit_synced(c, c->scratch, P));
    hipStream_t st = c->stream;
    if (!from_bam) {
        TRY(h2d(c, c->sp.off, in->ent_off, (n + 1) * 8)); TRY(h2d(c, c->sp.len, in->read_len, n * 8));
        TRY(h2d(c, c->sp.c0, in->c0, ne * 8)); TRY(h2d(c, c->sp.c1, in->c1, ne * 8)); TRY(h2d(c, c->sp.f0, in->f0, ne * 8)); TRY(h2d(c, c->sp.f1, in->f1, ne * 8));
        TRY(h2d(c, c->sp.chr, in->chr, ne * 4)); TRY(h2d(c, c->sp.mapq, in->mapq, ne * 4)); TRY(h2d(c, c->sp.strand, in->strand, ne)); TRY(h2d(c, c->sp.primary, in->primary, ne));
    }
    SplitArgs A{};
    A.n_reads = n; A.ent_off = dp<i64>(c->sp.off); A.read_len = dp<i64>(c->sp.len);
    A.c0 = dp<i64>(c->sp.c0); A.c1 = dp<i64>(c->sp.c1); A.f0 = dp<i64>(c->sp.f0); A.f1 = dp<i64>(c->sp.f1);
    A.chr = dp<int>(c->sp.chr); A.mapq = dp<int>(c->sp.mapq); A.strand = dp<uint8_t>(c->sp.strand); A.primary = dp<uint8_t>(c->sp.primary);
    if (from_bam) {
        A.ent_off = dp<i64>(c->sa.entoff); A.read_len = dp<i64>(c->sa.readlen);
        A.c0 = dp<i64>(c->sa.c0); A.c1 = dp<i64>(c->sa.c1); A.f0 = dp<i64>(c->sa.f0); A.f1 = dp<i64>(c->sa.f1);
        A.chr = dp<int>(c->sa.chr); A.mapq = dp<int>(c->sa.mapq); A.strand = dp<uint8_t>(c->sa.strand); A.primary = dp<uint8_t>(c->sa.primary);
    }
    A.sv = in->sv_size; A.max_size = in->max_size; A.min_mapq = in->min_mapq; A.parts = in->max_split_parts;
    A.seg = dp<SpSeg>(c->sp.seg); A.cnt = dp<int4>(c->sp.cnt); A.cap = cap;
    A.kind = dp<uint8_t>(c->sp.kind); A.read = dp<int>(c->sp.read); A.o_chr = dp<int>(c->sp.ochr); A.aux = dp<int>(c->sp.aux);
    A.a = dp<i64>(c->sp.a); A.b = dp<i64>(c->sp.b); A.c = dp<i64>(c->sp.c); A.d = dp<i64>(c->sp.d);
    const int grid = div_up(n, 256);
    TwoPhaseTimer T{c};
    TRY(T.count_begin());
    hipLaunchKernelGGL(k_split_count, dim3(grid), dim3(256), 0, st, A);
    scan_counts(st, ScanArgs{n, A.cnt, dp<i64>(c->sp.tiles), dp<i64>(c->sp.tot)});
    TRY(T.count_end());
    i64 tot[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(tot, c->sp.tot.p, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    out->n = tot[0];
    if (tot[0] > out->cap) return fail(c, CSV_E_CAPACITY, "need %lld candidates", (long long)tot[0]);
    if (tot[0] < 0 || tot[0] > cap_max) return fail(c, CSV_E_INVALID, "split-read analysis: inconsistent count (%lld candidates of %lld entries)", (long long)tot[0], (long long)ne);
    TRY(T.emit_begin());
    hipLaunchKernelGGL(k_split_emit, dim3(grid), dim3(256), 0, st, A);
    TRY(T.emit_end());
    const bool to_pool = (in->flags & CSV_CG_TO_POOL) != 0;
    if (to_pool && tot[0] > 0) {
        // (CSV_SP_FROM_BAM: a row's read is the call's RECORD - the index space of the CIGAR scan's rows of the chunk - and the
        // query length is the decode's, which is what read_len holds per call)
        PoolCols PC;
        TRY(pool_attach(c, in->read_base, from_bam ? c->bm.n : n, tot[0], &PC));
        const bool own_qlen = in->query_len && !from_bam;
        if (own_qlen) { TRY(reserve(c, c->sp.qlen, (size_t)n * 4)); TRY(h2d(c, c->sp.qlen, in->query_len, n * 4)); }
        PoolSegBase SB{};
        for (int k = 0; k < 5; k++) SB.b[k] = in->pool_seg_base[k];
        hipLaunchKernelGGL(k_pool_from_split, dim3(div_up(tot[0], 256)), dim3(256), 0, st, PC, c->pool.n, A, tot[0], SB, in->read_base,
                           own_qlen ? dp<int>(c->sp.qlen) : nullptr, from_bam ? dp<int>(c->sa.callrec) : nullptr);
        HIP_TRY(c, hipGetLastError());
        if (seq_to_pool) {
            const SeqReads SR{dp<uint8_t>(c->seq.rbytes), dp<i64>(c->seq.roff), dp<int>(c->seq.rlen), c->seq.n_reads};
            const SeqSplitSrc Q{from_bam ? dp<int>(c->sa.callrec) : nullptr, from_bam ? dp<int>(c->bm.flag) : nullptr, from_bam ? nullptr : dp<uint8_t>(c->seq.qrev)};
            const i64 base = c->pool.n;
            TRY(seq_attach(c, tot[0], tot[0],
                           [&](int4* cnt, int* err) { hipLaunchKernelGGL(k_seq_plan_split, dim3(div_up(tot[0], 256)), dim3(256), 0, st, SR, A, Q, tot[0], dp<int>(c->pool.aux) + base, cnt, err); },
                           [&](const int4* cnt, SeqPool SP, i64 blob_base) { hipLaunchKernelGGL(k_seq_gather_split, dim3(div_up(tot[0], 4)), dim3(256), 0, st, SR, SP, A, Q, tot[0], cnt, base, blob_base); }));
        }
        c->pool.n += tot[0];
    }
    // (with CSV_CG_TO_POOL an output array that is NULL is not written)
    const HostCol cols[] = {{out->kind, &c->sp.kind, tot[0]}, {out->read, &c->sp.read, tot[0] * 4}, {out->chr, &c->sp.ochr, tot[0] * 4}, {out->aux, &c->sp.aux, tot[0] * 4},
                            {out->a, &c->sp.a, tot[0] * 8}, {out->b, &c->sp.b, tot[0] * 8}, {out->c, &c->sp.c, tot[0] * 8}, {out->d, &c->sp.d, tot[0] * 8}};
    for (const HostCol& o : cols) TRY(d2h(c, o.host, *o.dev, o.bytes, !to_pool));
    HIP_TRY(c, hipStreamSynchronize(st));
    TRY(T.elapsed(&out->ms_device));
    return CSV_OK;
}

}  // extern "C"
