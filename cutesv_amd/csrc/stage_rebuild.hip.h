// stage_rebuild.hip.h — csv_rebuild_signatures (and csv_rebuild_route): rows (the caller's or the pool's) -> sorted, de-duplicated signature
// columns (RebuildState in ctx.hip.h, kernels in sort.hip.h).  Host code; included by cutesv_hip.hip.
extern "C" {

int csv_rebuild_signatures(csv_ctx* c, const csv_rebuild_in* in, csv_rebuild_out* out)
{
    if (!c || !in || !out) return CSV_E_INVALID;
    RebuildState& rb = c->rb;
    c->vs.stale();                                          // (whatever an earlier rebuild kept is no longer this call's)
    HIP_TRY(c, hipSetDevice(c->device));
    const bool from_pool = (in->flags & CSV_RB_FROM_POOL) != 0;
    const i64 n = from_pool ? c->pool.n : in->n;
    out->n_out = 0; out->ms_device = 0; out->n_passes = 0;
    if (n < 0 || n >= (1ll << 31) - 4096 || in->n_seg <= 0) return fail(c, CSV_E_INVALID, "bad rebuild input");
    // CSV_RB_RANK_FROM_NAMES: the ranks are the name pool's, in device memory already (computed now if an append made them stale)
    const bool by_name = from_pool && (in->flags & CSV_RB_RANK_FROM_NAMES) != 0;
    if ((in->flags & CSV_RB_RANK_FROM_NAMES) && !from_pool) return fail(c, CSV_E_INVALID, "CSV_RB_RANK_FROM_NAMES needs CSV_RB_FROM_POOL");
    if (from_pool && ((!by_name && (!in->read_rank || in->n_rank <= 0)) || !in->seg_aux_major)) return fail(c, CSV_E_INVALID, "CSV_RB_FROM_POOL needs read_rank");
    // CSV_RB_TIES_FROM_SEQS: the INS tie groups are settled from the context's sequence pool instead of by the caller
    const bool ties_from_seqs = (in->flags & CSV_RB_TIES_FROM_SEQS) != 0;
    if (ties_from_seqs && (!from_pool || !in->seg_nodedup || in->tie_order))
        return fail(c, CSV_E_INVALID, "CSV_RB_TIES_FROM_SEQS needs CSV_RB_FROM_POOL and seg_nodedup, and excludes tie_order");
    const bool want_ties = (in->tie_order || ties_from_seqs) && in->seg_nodedup;
    if (n == 0) return CSV_OK;
    if (by_name) {
        if (c->nm.n == 0) return fail(c, CSV_E_INVALID, "CSV_RB_RANK_FROM_NAMES: the name pool is empty");
        TRY(name_ranks_impl(c));
    }
    const int* d_rank = by_name ? dp<int>(c->nm.rank) : nullptr;
    const i64 n_rank = by_name ? c->nm.n : in->n_rank;
    // key widths (bits that are non-zero somewhere) and the validity of every row: found on the device, behind the upload (r04
    // walked the columns on the host first: ~3 ms for a 30x genome's 2.85 M rows, in front of a 0.5 ms sort)
    i64 mx_a = 0, mx_b = 0; int mx_rid = 0, mx_aux = 0, mx_seg = 0, mx_aux_all = 0;
    auto nbytes = [](u64 v) { int k = 0; while (v) { k++; v >>= 8; } return k; };
    auto nbits = [](u64 v) { int k = 0; while (v) { k++; v >>= 1; } return k; };
    const int nunits = div_up(n, SORT_WTILE), nblk = div_up(nunits, 4), ntile = div_up(n, 2048);
    Plan P;
    P.add(rb.seg, n * 4); P.add(rb.a, n * 8); P.add(rb.b, n * 8); P.add(rb.rid, n * 4); P.add(rb.aux, n * 4); P.add(rb.auxk, n * 4);
    P.add(rb.major, in->n_seg); P.add(rb.nodedup, in->n_seg); P.add(rb.perm0, n * 4); P.add(rb.perm1, n * 4); P.add(rb.hist, (size_t)RS_RADIX * nunits * 4);
    P.add(rb.tot, RS_RADIX * 4); P.add(rb.partial, (ntile + 2) * 4);
    P.add(rb.el0, (size_t)n * 32); P.add(rb.el1, (size_t)n * 32);          // composite-key elements (16 or 32 bytes each; sized for either)
    P.add(rb.oseg, n * 4); P.add(rb.oa, n * 8); P.add(rb.ob, n * 8); P.add(rb.orid, n * 4); P.add(rb.oaux, n * 4); P.add(rb.osrc, n * 4); P.add(rb.segcnt, ((size_t)in->n_seg + 2) * 8);
    if (from_pool && !by_name) P.add(rb.rank, (size_t)in->n_rank * 4);
    P.add(rb.mx, 64);
    if (want_ties) P.add(rb.drop, n + 64);
    TRY(commit_synced(c, c->scratch, P));
    hipStream_t st = c->stream;
    TRY(h2d(c, rb.major, in->seg_aux_major, in->n_seg));
    if (in->seg_nodedup) TRY(h2d(c, rb.nodedup, in->seg_nodedup, in->n_seg));
    if (!from_pool) {
        TRY(h2d(c, rb.seg, in->seg_id, n * 4)); TRY(h2d(c, rb.a, in->a, n * 8)); TRY(h2d(c, rb.b, in->b, n * 8));
        TRY(h2d(c, rb.rid, in->read_id, n * 4)); TRY(h2d(c, rb.aux, in->aux, n * 4));
    }
    // the rows -> the input columns (pool rows: read index -> name rank; host rows: in place), the key widths from the device
    if (from_pool && !by_name) {
        TRY(h2d(c, rb.rank, in->read_rank, in->n_rank * 4));
        d_rank = dp<int>(rb.rank);
    }
    HIP_TRY(c, hipMemsetAsync(rb.mx.p, 0, 64, st));
    const PoolState& pl = c->pool;
    hipLaunchKernelGGL(k_pool_to_rows, dim3(div_up(n, 2048)), dim3(256), 0, st, dp<int>(from_pool ? pl.seg : rb.seg), dp<i64>(from_pool ? pl.a : rb.a), dp<i64>(from_pool ? pl.b : rb.b),
                       dp<int>(from_pool ? pl.read : rb.rid), dp<int>(from_pool ? pl.aux : rb.aux), n, from_pool ? d_rank : (const int*)nullptr, from_pool ? n_rank : (i64)0, in->n_seg,
                       dp<uint8_t>(rb.major), dp<int>(rb.seg), dp<i64>(rb.a), dp<i64>(rb.b), dp<int>(rb.rid), dp<int>(rb.aux), dp<unsigned long long>(rb.mx));
    unsigned long long mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(mx, rb.mx.p, 56, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (mx[5]) return fail(c, CSV_E_INVALID, from_pool ? "a pool row has a negative key, a segment out of range or a read without a rank"
                                                      : "a row has a negative key or a segment out of range");
    mx_a = (i64)mx[0]; mx_b = (i64)mx[1]; mx_rid = (int)mx[2]; mx_aux = (int)mx[3]; mx_seg = (int)mx[4]; mx_aux_all = (int)mx[6];
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    // the composite-key sort (sort.hip.h) whenever the key fits 128 bits; CSV_RB_PERM_SORT=1 forces the permutation sort
    KeyLayout KL{};
    KL.ib = nbits((u64)(n - 1)) > 0 ? nbits((u64)(n - 1)) : 1;
    KL.rb = nbits((u64)mx_rid) > 0 ? nbits((u64)mx_rid) : 1; KL.bb = nbits((u64)mx_b) > 0 ? nbits((u64)mx_b) : 1;
    KL.ab = nbits((u64)mx_a) > 0 ? nbits((u64)mx_a) : 1; KL.xb = nbits((u64)mx_aux); KL.sb = nbits((u64)mx_seg) > 0 ? nbits((u64)mx_seg) : 1;
    KL.pb = nbits((u64)mx_aux_all);
    KL.T = KL.rb + KL.bb + KL.ab + KL.xb + KL.sb;
    // (the compact element holds aux | key | index in 128 bits; with no aux bits and ib + T == 128 its shifts would be by 128: wide then)
    KL.wide = (KL.ib + KL.T + KL.pb <= 128 && KL.ib + KL.T < 128) ? 0 : 1;
    const bool composite = KL.T <= 128 && !getenv("CSV_RB_PERM_SORT");
    RebuildArgs R{};
    R.n = n;
    R.seg = dp<int>(rb.seg); R.a = dp<i64>(rb.a); R.b = dp<i64>(rb.b); R.rid = dp<int>(rb.rid); R.aux = dp<int>(rb.aux);
    R.auxk = dp<int>(rb.auxk); R.keep = nullptr; R.partial = dp<int>(rb.partial);
    R.nodedup = in->seg_nodedup ? dp<uint8_t>(rb.nodedup) : nullptr;
    R.o_seg = dp<int>(rb.oseg); R.o_a = dp<i64>(rb.oa); R.o_b = dp<i64>(rb.ob); R.o_rid = dp<int>(rb.orid);
    R.o_aux = dp<int>(rb.oaux); R.o_src = dp<int>(rb.osrc); R.n_out = (int*)((char*)c->res.cnt.p + 768);      // (a word of its own: the run arenas at +0 / +256 may have a publish in flight)
    R.drop = nullptr;
    out->n_tie_rows = 0; out->n_tie_dropped = 0;
    bool ties_settled = false;
    int npass = 0;
    // the tie groups' round trip to the caller (csv_tie_order_fn) or, CSV_RB_TIES_FROM_SEQS, to k_seq_tie_order: `lst` = {position | continues << 31, source row}, any order
    std::vector<int> tie_pos, tie_src; std::vector<uint8_t> tie_flag;
    auto ask_caller = [&](std::vector<int2>& lst) -> int {
        const int n_list = (int)lst.size();
        std::sort(lst.begin(), lst.end(), [](const int2& x, const int2& y) { return (x.x & 0x7fffffff) < (y.x & 0x7fffffff); });
        std::vector<int64_t> goff;
        std::vector<int> src((size_t)n_list), order((size_t)n_list, -1);
        std::vector<uint8_t> drop((size_t)n_list, 0);
        tie_pos.assign((size_t)n_list, 0); tie_src.assign((size_t)n_list, 0); tie_flag.assign((size_t)n_list, 0);
        for (int k = 0; k < n_list; k++) {
            if (!(lst[k].x & (int)0x80000000)) goff.push_back(k);               // a group's head
            tie_pos[k] = lst[k].x & 0x7fffffff; src[k] = lst[k].y;
        }
        goff.push_back(n_list);
        if (ties_from_seqs) TRY(seq_tie_order(c, (i64)goff.size() - 1, goff.data(), src.data(), n_list, order.data(), drop.data()));
        else {
            const int rc = in->tie_order(in->tie_user, (int64_t)goff.size() - 1, goff.data(), src.data(), order.data(), drop.data());
            if (rc != 0) return fail(c, CSV_E_INVALID, "tie_order returned %d", rc);
        }
        std::vector<uint8_t> seen((size_t)n_list, 0);
        int64_t dropped = 0;
        for (size_t g = 0; g + 1 < goff.size(); g++) {                            // order[] must be a permutation inside every group
            const int64_t g0 = goff[g], g1 = goff[g + 1];
            for (int64_t k = g0; k < g1; k++) {
                const int64_t o = order[k];
                if (o < 0 || o >= g1 - g0 || seen[g0 + o]) return fail(c, CSV_E_INVALID, "tie_order: order[] is not a permutation inside group %zu", g);
                seen[g0 + o] = 1;
                tie_src[g0 + o] = src[k]; tie_flag[g0 + o] = drop[k] ? 1 : 0;
                dropped += drop[k] ? 1 : 0;
            }
        }
        out->n_tie_rows = n_list; out->n_tie_dropped = dropped;
        return CSV_OK;
    };
    // INS rows that tie on their integer keys: the caller orders them (by sequence) and names the duplicates; the answer is
    // written into the sorted elements / the permutation and a drop map on the device, and the gather never knows.  The output
    // buffers are free until the gather: oa holds the list `find` makes, oseg / orid / ob the answer on its way back to `apply`.
    auto settle_ties = [&](auto find, auto apply) -> int {
        int* d_n = R.n_out;
        HIP_TRY(c, hipMemsetAsync(d_n, 0, 4, st));
        HIP_TRY(c, hipMemsetAsync(rb.drop.p, 0, (size_t)n, st));
        find((int2*)rb.oa.p, d_n);
        int n_list = 0;
        HIP_TRY(c, hipMemcpyAsync(&n_list, d_n, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (n_list > 0) {
            std::vector<int2> lst((size_t)n_list);
            HIP_TRY(c, hipMemcpy(lst.data(), rb.oa.p, (size_t)n_list * 8, hipMemcpyDeviceToHost));
            TRY(ask_caller(lst));
            TRY(h2d(c, rb.oseg, tie_pos.data(), (i64)n_list * 4)); TRY(h2d(c, rb.orid, tie_src.data(), (i64)n_list * 4)); TRY(h2d(c, rb.ob, tie_flag.data(), n_list));
            apply(n_list);
            HIP_TRY(c, hipStreamSynchronize(st));                                       // (the host vectors are the copies' sources)
        }
        ties_settled = true;
        return CSV_OK;
    };
    if (composite) {
        RsCols C{dp<int>(rb.seg), dp<i64>(rb.a), dp<i64>(rb.b), dp<int>(rb.rid), dp<int>(rb.aux), dp<uint8_t>(rb.major)};
        void* e_in = rb.el0.p; void* e_out = rb.el1.p;
        auto run_sort = [&](auto wide_tag) -> int {
            constexpr bool W = decltype(wide_tag)::value;
            typedef RsElem<W> E;
            hipLaunchKernelGGL(k_rs_pack<W>, dim3(div_up(n, 256)), dim3(256), 0, st, C, n, KL, (E*)e_in);
            for (int shift = 0; shift < KL.T; shift += RS_BITS) {
                const int dbits = KL.T - shift < RS_BITS ? KL.T - shift : RS_BITS;
                hipLaunchKernelGGL(k_rs_hist<W>, dim3(nblk), dim3(256), 0, st, (const E*)e_in, n, nunits, KL, shift, dbits, dp<int>(rb.hist));
                hipLaunchKernelGGL(k_sort_rowsum, dim3(RS_RADIX), dim3(256), 0, st, dp<int>(rb.hist), nunits, dp<int>(rb.tot));
                hipLaunchKernelGGL(k_sort_rowscan, dim3(RS_RADIX), dim3(256), 0, st, dp<int>(rb.hist), nunits, dp<int>(rb.tot));
                hipLaunchKernelGGL(k_rs_scatter<W>, dim3(nblk), dim3(256), 0, st, (const E*)e_in, (E*)e_out, n, nunits, KL, shift, dbits, dp<int>(rb.hist));
                std::swap(e_in, e_out);
                npass++;
            }
            RsTail T{};
            T.n = n; T.L = KL; T.nodedup = R.nodedup; T.drop = nullptr; T.partial = R.partial;
            T.o_seg = R.o_seg; T.o_a = R.o_a; T.o_b = R.o_b; T.o_rid = R.o_rid; T.o_aux = R.o_aux; T.o_src = R.o_src; T.n_out = R.n_out;
            if (want_ties) {
                TRY(settle_ties([&](int2* lst, int* d_n) { hipLaunchKernelGGL(k_rs_ties<W>, dim3(div_up(n, 256)), dim3(256), 0, st, T, (const E*)e_in, lst, d_n); },
                                [&](int n_list) { hipLaunchKernelGGL(k_rs_tie_apply<W>, dim3(div_up(n_list, 256)), dim3(256), 0, st, n_list, dp<int>(rb.oseg), dp<int>(rb.orid),
                                                                     dp<uint8_t>(rb.ob), dp<int>(rb.aux), KL, (E*)e_in, dp<uint8_t>(rb.drop)); }));
                T.drop = dp<uint8_t>(rb.drop);
            }
            hipLaunchKernelGGL(k_rs_count<W>, dim3(ntile), dim3(256), 0, st, T, (const E*)e_in);
            hipLaunchKernelGGL(k_rs_apply<W>, dim3(ntile), dim3(256), 0, st, T, (const E*)e_in);
            return CSV_OK;
        };
        TRY(KL.wide ? run_sort(std::true_type{}) : run_sort(std::false_type{}));
    } else {
        hipLaunchKernelGGL(k_rebuild_auxkey, dim3(div_up(n, 256)), dim3(256), 0, st, n, dp<int>(rb.seg), dp<int>(rb.aux),
                           dp<uint8_t>(rb.major), dp<int>(rb.auxk));
        // least significant key first: read_id, b, a, [aux], segment
        const SortField fields[5] = {{rb.rid.p, 0, 0, nbytes((u64)mx_rid), ~0u}, {rb.b.p, 1, 0, nbytes((u64)mx_b), ~0u}, {rb.a.p, 1, 0, nbytes((u64)mx_a), ~0u},
                                     {rb.auxk.p, 0, 0, nbytes((u64)mx_aux), ~0u}, {rb.seg.p, 0, 0, nbytes((u64)mx_seg) > 0 ? nbytes((u64)mx_seg) : 1, ~0u}};
        R.perm = sort_passes(st, fields, 5, n, nunits, dp<int>(rb.perm0), dp<int>(rb.perm1), dp<int>(rb.hist), dp<int>(rb.tot), &npass);
        if (want_ties) {
            TRY(settle_ties([&](int2* lst, int* d_n) { hipLaunchKernelGGL(k_rebuild_ties, dim3(div_up(n, 256)), dim3(256), 0, st, R, lst, d_n); },
                            [&](int n_list) { hipLaunchKernelGGL(k_rebuild_tie_apply, dim3(div_up(n_list, 256)), dim3(256), 0, st, n_list, dp<int>(rb.oseg), dp<int>(rb.orid),
                                                                 dp<uint8_t>(rb.ob), const_cast<int*>(R.perm), dp<uint8_t>(rb.drop)); }));
            R.drop = dp<uint8_t>(rb.drop);
        }
        hipLaunchKernelGGL(k_rebuild_count, dim3(ntile), dim3(256), 0, st, R);
        hipLaunchKernelGGL(k_rebuild_apply, dim3(ntile), dim3(256), 0, st, R);
    }
    // rows per segment and the INS tie count ([n_seg] = ties), from the sorted output
    HIP_TRY(c, hipMemsetAsync(dp<i64>(rb.segcnt) + in->n_seg, 0, 8, st));
    // (the tie count is a grid-stride loop over the sorted rows: enough workgroups for ~4 rows per thread)
    const int g_sc = std::max(div_up(in->n_seg, 256), std::min(div_up(n, 1024), 8192));
    if (ties_settled) R.nodedup = nullptr;                  // (nothing left to count)
    hipLaunchKernelGGL(k_rebuild_segcount, dim3(g_sc), dim3(256), 0, st, R, in->n_seg,
                       dp<i64>(rb.segcnt), dp<i64>(rb.segcnt) + in->n_seg);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    int n_out = 0;
    std::vector<i64> segcnt((size_t)in->n_seg + 1);
    HIP_TRY(c, hipMemcpyAsync(&n_out, (char*)c->res.cnt.p + 768, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(segcnt.data(), rb.segcnt.p, ((size_t)in->n_seg + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipEventElapsedTime(&out->ms_device, c->ev[0], c->ev[1]));
    out->n_out = n_out; out->n_passes = npass;
    out->n_ins_ties = ties_settled ? 0 : segcnt[(size_t)in->n_seg];
    if (out->seg_count) memcpy(out->seg_count, segcnt.data(), (size_t)in->n_seg * 8);
    const bool keep_dev = (in->flags & CSV_RB_KEEP_ON_DEVICE) != 0;
    out->dev_seg_id = out->dev_a = out->dev_b = out->dev_read_id = out->dev_aux = out->dev_src_row = nullptr;
    if (keep_dev) {
        out->dev_seg_id = rb.oseg.p; out->dev_a = rb.oa.p; out->dev_b = rb.ob.p; out->dev_read_id = rb.orid.p;
        out->dev_aux = rb.oaux.p; out->dev_src_row = rb.osrc.p;
    }
    // (with CSV_RB_KEEP_ON_DEVICE a NULL host array is simply not filled; without the flag all six are required, as before)
    const HostCol cols[] = {{out->seg_id, &rb.oseg, (i64)n_out * 4}, {out->a, &rb.oa, (i64)n_out * 8}, {out->b, &rb.ob, (i64)n_out * 8},
                            {out->read_id, &rb.orid, (i64)n_out * 4}, {out->aux, &rb.oaux, (i64)n_out * 4}, {out->src_row, &rb.osrc, (i64)n_out * 4}};
    for (const HostCol& o : cols) TRY(d2h(c, o.host, *o.dev, o.bytes, !keep_dev));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->bt.uploaded = c->bt.ran = false;          // cnt was used as scratch
    rb.route = !composite ? 3 : KL.wide ? 2 : 1;
    if (from_pool && keep_dev) { c->vs.kept = c->vs.gen; c->vs.n_out = n_out; c->vs.by_name = by_name; }      // (csv_seq_alt_gather / csv_name_support_join)
    return CSV_OK;
}

int csv_rebuild_route(const csv_ctx* c) { return c ? c->rb.route : 0; }

}  // extern "C"
