// stage_run.hip.h — engine, the run: csv_batch_run, csv_batch_validate and the one-shot csv_cluster_batch.  run_impl queues the
// clustering chain, the reads stage and the genotype kernels of the resident batch (BatchState) into the result arena that is
// not the last run's (ResultState); read_counters fetches the counters and re-runs a batch whose reads table needs the general
// sort.  Nothing here reads the environment: c->opt is loaded by the upload.  Host code only.
namespace {

// workgroups of k_genotype<1024,4>: about two resident sets - calls differ a lot in cost, and workgroups that start as others
// finish even the tail out (measured on the 90x workload: 1536..2048 -> 82-86 us, 4096..8192 -> 76 us, 16384 -> 80 us)
constexpr int GT_GRID = 4096;

int read_counters(csv_ctx* c);

// general stable sort of the reads table by (chromosome, start): the fallback of the reads_order stage for tables that
// are not a permutation of disjoint sorted runs.  LSD radix passes of sort.hip.h over the 5 start bytes and the
// chromosome bytes; the result is a row permutation that k_reads_gather applies.
int general_reads_sort(csv_ctx* c, hipStream_t st)
{
    const i64 R = c->bt.n_reads;
    const int nunits = div_up(R, SORT_WTILE);
    int rc;
    if ((rc = reserve(c, c->ro.gs_chrom, R * 4)) || (rc = reserve(c, c->ro.gs_perm0, R * 4)) || (rc = reserve(c, c->ro.gs_perm1, R * 4)) ||
        (rc = reserve(c, c->ro.gs_hist, (size_t)256 * nunits * 4)) || (rc = reserve(c, c->ro.gs_tot, 256 * 4))) return rc;
    hipLaunchKernelGGL(k_reads_chromcol, dim3(div_up(R, 256)), dim3(256), 0, st, c->bt.B, dp<int>(c->ro.gs_chrom));
    int cbytes = 0;
    for (u64 v = (u64)(c->bt.B.n_chrom > 0 ? c->bt.B.n_chrom - 1 : 0); v; v >>= 8) cbytes++;
    // starts < 2^40 (checked with the ends by k_reads_gather): five key bytes, of which int32 starts have four
    const bool rn = c->bt.B.r_start.p32 != nullptr;
    const SortField fields[2] = {{rn ? (const void*)c->bt.B.r_start.p32 : (const void*)c->bt.B.r_start.p64, rn ? 0 : 1, 0, 5, rn ? 0x0fu : 0x1fu},
                                 {c->ro.gs_chrom.p, 0, 0, cbytes, ~0u}};
    c->bt.B.ro_perm = sort_passes(st, fields, 2, R, nunits, dp<int>(c->ro.gs_perm0), dp<int>(c->ro.gs_perm1), dp<int>(c->ro.gs_hist), dp<int>(c->ro.gs_tot), nullptr);
    HIP_TRY(c, hipGetLastError());
    return CSV_OK;
}

int run_impl(csv_ctx* c, csv_run_stats* stats)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBatch& B = c->bt.B;
    const i64 W = B.W;
    constexpr int LDS_SMALL = refine_lds_bytes<64>();
    constexpr int LDS_MID = refine_lds_bytes<256>();
    constexpr int LDS_BIG = refine_lds_bytes<2048>();
    constexpr int LDS_PLAN = rp_lds_bytes(RO_CAP);
    if (!c->lds_set) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_refine<256, 2048, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BIG));
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_reads_plan<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_PLAN));
        HIP_TRY(c, hipFuncSetAttribute((const void*)k_reads_plan<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_PLAN));
        c->lds_set = true;
    }
    int ev = 0;
    auto mark = [&]() -> hipError_t { return stats ? hipEventRecord(c->ev[ev++], st) : hipSuccess; };
    const auto& O = c->opt;
    const bool dbg = O.debug;
#define DBG(name)                                                                                          \
    do {                                                                                                   \
        if (dbg) {                                                                                         \
            fprintf(stderr, "[csv] %s ...", name); fflush(stderr);                                         \
            hipError_t e_ = hipDeviceSynchronize();                                                        \
            fprintf(stderr, " %s\n", hipGetErrorString(e_)); fflush(stderr);                               \
        }                                                                                                  \
    } while (0)
    // this run's result arena: the other one than the last run's (whose publish may still be reading it on the publish stream)
    {
        const int p = c->res.parity ^ 1;
        if (c->res.pend[p].live) HIP_TRY(c, hipStreamWaitEvent(st, c->res.ev_pub[p], 0));       // (launched two runs ago)
        c->res.parity = p;
        B.cnt = (DevCounters*)((char*)c->res.cnt.p + 256 * p);
        B.o_rec = p ? dp<CallRec>(c->res.o_rec2) : dp<CallRec>(c->res.o_rec);
        B.o_supsig = p ? dp<int>(c->res.o_supsig2) : dp<int>(c->res.o_supsig);
    }
    HIP_TRY(c, mark());
    if (W == 0) HIP_TRY(c, hipMemsetAsync(B.cnt, 0, sizeof(DevCounters), st));      // otherwise k_chain_count zeroes them
    HIP_TRY(c, mark());                                                              // slot 0: init (empty batch only)
    // Plain runs fork the independent kernels onto side streams (joined again before k_items_scan /
    // k_genotype); instrumented runs (stats != NULL) and CSV_DEBUG keep everything on the main stream so
    // that every kernel is timed alone.
    // (forking costs a few event waits: only worth it when the batch has pair types or genotyping)
    const bool do_gt = c->bt.any_genotype && B.n_reads > 0;
    // the packed table of an upload does not change between runs: a resident re-run keeps it (csv_batch_option) and has no reads stage
    const bool keep_reads = c->ro.reads_ready && c->ro.reuse_reads && !stats;
    const bool fork = !stats && !dbg && !O.no_fork && (c->bt.any_pair || (do_gt && !keep_reads) || O.fork_always);
    // A genotyping batch has two producer chains - clustering (k_chain_count .. k_emit) and the reads stage - that meet in
    // k_genotype.  A wait across queues costs 6-11 us when the event fires late and next to nothing when it fired long ago,
    // so the LONGER chain stays on the main stream together with the genotype kernels and the shorter one is forked off:
    // its completion event has long fired when the main stream gets there.  (Reads dominate a 30x HiFi genome, clustering a
    // 90x all-types one.)  `st` is the stream of the clustering chain from here on, `sM` the main stream.
    hipStream_t sM = c->stream;
    const bool swap = fork && do_gt && !keep_reads && !c->bt.copies_pending && B.n_reads > 4 * W && W > 0 && !O.no_swap;
    if (swap) st = c->side[2];
    hipStream_t sB = fork ? c->side[0] : st, sC = fork ? c->side[1] : st, sD = swap ? sM : (fork ? c->side[2] : st);
#define LAUNCH_ON(strm, name, kern, grid, block, lds, ...)                             \
    do {                                                                               \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, strm, __VA_ARGS__);      \
        DBG(name);                                                                     \
        HIP_TRY(c, mark());                                                            \
    } while (0)
#define LAUNCH(name, kern, grid, block, lds, ...) LAUNCH_ON(st, name, kern, grid, block, lds, __VA_ARGS__)
    // s_early: the stream the upload decoded the start column on (a one-shot call whose reads table came in its 16-bit forms):
    // k_reads_runs / k_reads_plan read the starts and nothing else of the table, so they run there, behind the decode, while the
    // end column is still on the link; s2 waits for their event before it packs the table
    auto reads_stage = [&](hipStream_t s2, hipStream_t s_early = nullptr) -> int {       // reads order + pack + longest read per chromosome on stream s2
        const int nr = div_up(B.n_reads, 2048);
        const bool rn = B.r_start.p32 != nullptr;
        const bool keep = keep_reads;
        if (!keep) {                                      // (k_reads_plan leaves a state on every path; nothing to reset)
            if (B.ro_mode == 2) {
                const int rc = general_reads_sort(c, s2);
                if (rc) return rc;
            } else if (B.ro_mode == 1) {
                const hipStream_t so = s_early ? s_early : s2;
                if (rn) {
                    hipLaunchKernelGGL(k_reads_runs<true>, dim3(div_up(B.n_reads, RO_TILE)), dim3(256), 0, so, B);
                    hipLaunchKernelGGL(k_reads_plan<true>, dim3(1), dim3(RP_THREADS), LDS_PLAN, so, B);
                } else {
                    hipLaunchKernelGGL(k_reads_runs<false>, dim3(div_up(B.n_reads, RO_TILE)), dim3(256), 0, so, B);
                    hipLaunchKernelGGL(k_reads_plan<false>, dim3(1), dim3(RP_THREADS), LDS_PLAN, so, B);
                }
                if (s_early) { HIP_TRY(c, hipEventRecord(c->ev_rd[4], so)); HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_rd[4], 0)); }
            }
        }
        DBG("reads_order");
        if (s2 == st || stats) HIP_TRY(c, mark());
        if (!keep) {
            if (rn) hipLaunchKernelGGL(k_reads_gather<true>, dim3(nr), dim3(256), 0, s2, B);
            else hipLaunchKernelGGL(k_reads_gather<false>, dim3(nr), dim3(256), 0, s2, B);
        }
        DBG("reads_gather");
        if (s2 == st || stats) HIP_TRY(c, mark());
        if (!keep) hipLaunchKernelGGL(k_reads_maxlen, dim3(B.n_chrom < 1024 ? (B.n_chrom > 0 ? B.n_chrom : 1) : 1024), dim3(256), 0, s2, B);
        DBG("reads_maxlen");
        if (s2 == st || stats) HIP_TRY(c, mark());
        c->ro.reads_ready = true;
        return CSV_OK;
    };
    if (c->bt.copies_pending) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_copy[0], 0));       // positions, lengths, INV / TRA words
    bool zero_done = false;
    if (c->bt.unpack_pending) {                               // CSV_IN_SIG_DELTA16: the position column out of its gaps, first kernel of the call
        // (a gate-first call: the same kernel fetches `b` of the rows at position 0 - k_lazy_zero's whole job - as it writes them)
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_anc, 0));
        c->bt.unpack_args.zero_b = (c->bt.lazy_pending && W > 0) ? 1 : 0;
        zero_done = c->bt.unpack_args.zero_b != 0;
        hipLaunchKernelGGL(k_unpack_a16, dim3((unsigned)c->bt.unpack_tiles + 1), dim3(256), 0, st, c->bt.unpack_args, B);
        c->bt.unpack_pending = false;
    }
    // A run decides what it launches from what IT knows - nothing is carried over from earlier runs of the upload (r05 skipped
    // the tiers above 64 signatures when an earlier, identical run had found them empty: state only a benchmark loop has).  In
    // a one-shot call the column copies are still on the link when the chain kernels are queued, so the host can wait for
    // k_chain_apply's word {this run, work items above 64 signatures} - it arrives long before the copies end - and queue
    // only the tiers that have work; a resident run queues them all (an empty tier costs its launch, ~4.5 us).
    const bool peek = c->bt.copies_pending && c->h_flag && !O.no_peek && !stats && !dbg;
    B.host_flag = peek ? c->d_flag : nullptr;
    B.run_seq = ++c->run_seq;
    if (W > 0) {
        const int nb = div_up(W, CH_TILE);
        if (fork && do_gt && !keep_reads) {
            // reads order + pack: independent of the clustering kernels.  Either chain waits only for whatever ran before on
            // the main stream (the previous run's genotype / publish kernels read what this run rewrites).  The stage's
            // verdict on the table goes to the upload's state, not to the run's counters (which k_chain_count zeroes).
            HIP_TRY(c, hipEventRecord(c->ev_init, sM));
            HIP_TRY(c, hipStreamWaitEvent(swap ? st : sD, c->ev_init, 0));
            const bool early = c->ro.reads_early && c->bt.copies_pending && !swap && !O.no_reads_overlap;
            if (early) HIP_TRY(c, hipStreamWaitEvent(c->side[1], c->ev_init, 0));
            const int rc = reads_stage(sD, early ? c->side[1] : nullptr);
            c->ro.reads_early = false;
            if (rc) return rc;
            if (!swap) HIP_TRY(c, hipEventRecord(c->ev_aux[2], sD));
        }
        const bool lazy = c->bt.lazy_pending;                 // (the first run of a gate-first upload; stats are never taken on one)
        if (lazy && !zero_done) {
            const int gz = nb < 2048 ? nb : 2048;
            if (B.a.p32) hipLaunchKernelGGL(k_lazy_zero<true>, dim3(gz), dim3(256), 0, st, B);
            else hipLaunchKernelGGL(k_lazy_zero<false>, dim3(gz), dim3(256), 0, st, B);
        }
        if (B.a.p32) LAUNCH("chain_count", k_chain_count<true>, nb, 256, 0, B);
        else LAUNCH("chain_count", k_chain_count<false>, nb, 256, 0, B);
        LAUNCH("chain_apply", k_chain_apply, div_up(nb, 4), 256, 0, B);
        if (B.per_sig) hipLaunchKernelGGL(k_chain_ids, dim3(nb), dim3(256), 0, st, B);      // (optional outputs; timed with whatever follows)
        if (lazy) {
            if (B.a.p32) hipLaunchKernelGGL(k_lazy_fetch<true>, dim3(nb), dim3(256), 0, st, B);
            else hipLaunchKernelGGL(k_lazy_fetch<false>, dim3(nb), dim3(256), 0, st, B);
            DBG("lazy_fetch");
            // the device columns now hold every row a kernel reads: later runs of this upload (the general-sort re-run of a reads
            // table, a caller's csv_batch_run) take them as they are - the caller's host columns are not touched again
            c->bt.lazy_pending = false;
            B.h_b = nullptr; B.h_rid = nullptr; B.h_aux = nullptr; B.h_rows8 = nullptr; B.tile_lead = nullptr;
        }
        if (c->bt.copies_pending) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_copy[1], 0));   // read ids, INS sequence lengths
        int g_small = B.cap_items < 8192 ? B.cap_items : 8192;
        if (g_small < 1) g_small = 1;
        // (the resident set: CSV_IW_WAVES wavefronts per SIMD on every CU.  The units are dealt longest first, so a grid
        // that is resident at once finishes sooner than one whose last workgroups wait for a slot: 23.1 vs 23.5 us on cfg3
        // with 1536 vs 3072 workgroups)
        const int g_res = c->n_cu * CSV_IW_WAVES;
        int g_iw = div_up(B.cap_items, 4) < g_res ? div_up(B.cap_items, 4) : g_res;
        if (O.iw_grid > 0) g_iw = O.iw_grid;              // tuning aid
        if (g_iw < 1) g_iw = 1;
        // The tiers above 64 signatures usually have nothing to do (a 30x genome has no such cluster).  With the answer of THIS
        // run's k_chain_apply in hand (one-shot calls, see `peek` above) only the tiers with work are queued; the wait ends when
        // the position column has crossed the link and the two chain kernels have run, while the stream goes on to fetch / wait
        // for the other columns - it never runs dry because of it.  No answer within 20 ms: everything is queued.
        bool need_big = true;
        if (B.host_flag) {
            const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
            for (;;) {
                const unsigned long long w = *(volatile unsigned long long*)c->h_flag;
                if ((unsigned)(w >> 32) == (unsigned)B.run_seq) { need_big = (unsigned)w > 0; break; }
                if (std::chrono::steady_clock::now() > t_end) break;
                __builtin_ia32_pause();
            }
        }
        // The tiers run one after the other.  Side by side (CSV_TIER_FORK_MIN=<signatures>; the default for >= 4 Mi until r05) the
        // register tier and the one-wavefront tier - both bound by vector issue - share the CUs and finish when their sum would
        // have (r06 timeline of the 90x genome: 45 + 90 us overlapped = 99 us, against 37 + 61 in a row), and the fork and the
        // join add 8 + 14 us of event waits: 256.5 -> 246 us for the step without it.
        const bool tier_fork = fork && W >= (i64)O.tier_fork_min;
        // with clusters above 64 signatures in the batch, the one-wavefront tier for 65 .. 256 also takes the DUP / INV / TRA clusters
        // of at most 64 (its second phase): one grid, the long clusters first, instead of two kernels in a row
        B.pair_in_mid = (need_big && c->bt.any_pair && !O.no_pair_in_mid) ? 1 : 0;
        const bool side_b = tier_fork && need_big, side_c = tier_fork && c->bt.any_pair && !B.pair_in_mid;
        if (!tier_fork) { sB = st; sC = st; }
        if (side_b || side_c) {
            HIP_TRY(c, hipEventRecord(c->ev_sel, st));
            if (side_b) HIP_TRY(c, hipStreamWaitEvent(sB, c->ev_sel, 0));
            if (side_c) HIP_TRY(c, hipStreamWaitEvent(sC, c->ev_sel, 0));
        }
        if (B.a.p32) LAUNCH("refine_indel_wave", k_refine_indel_wave<true>, g_iw, 256, 0, B);
        else LAUNCH("refine_indel_wave", k_refine_indel_wave<false>, g_iw, 256, 0, B);
        if (c->bt.any_pair && !B.pair_in_mid) LAUNCH_ON(sC, "refine_wave", (k_refine<64, 64, false>), g_small, 64, LDS_SMALL, B, 0, 64);
        else HIP_TRY(c, mark());
        const int mid_cap = O.mid_grid > 0 ? O.mid_grid : 8192, big_cap = O.big_grid > 0 ? O.big_grid : 512;
        int g_mid = B.cap_items < mid_cap ? B.cap_items : mid_cap;
        if (g_mid < 1) g_mid = 1;
        int g_big = B.cap_items < big_cap ? B.cap_items : big_cap;
        if (g_big < 1) g_big = 1;
        if (need_big) {
            LAUNCH_ON(sB, "refine_mid", (k_refine<64, 256, true>), g_mid, 64, LDS_MID, B, 64, MID_CAP);
            LAUNCH_ON(sB, "refine_block", (k_refine<256, 2048, true>), g_big, 256, LDS_BIG, B, MID_CAP, 0x7fffffff);
        } else { HIP_TRY(c, mark()); HIP_TRY(c, mark()); }
        if (side_b) { HIP_TRY(c, hipEventRecord(c->ev_aux[0], sB)); HIP_TRY(c, hipStreamWaitEvent(st, c->ev_aux[0], 0)); }
        if (side_c) { HIP_TRY(c, hipEventRecord(c->ev_aux[1], sC)); HIP_TRY(c, hipStreamWaitEvent(st, c->ev_aux[1], 0)); }
        LAUNCH("items_scan", k_items_scan, B.cap_items / IS_CHUNK + 1, 64 * IS_NW, 0, B);
        LAUNCH("emit", k_emit, 2048, 256, 0, B);
        if (swap) {                                       // the clustering chain joins the main stream
            HIP_TRY(c, hipEventRecord(c->ev_aux[2], st));
            HIP_TRY(c, hipStreamWaitEvent(sM, c->ev_aux[2], 0));
            st = sM;
        }
        if (do_gt) {
            if (swap) {}
            else if (fork && !keep_reads) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_aux[2], 0));
            else { HIP_TRY(c, hipStreamWaitEvent(st, c->ev_reads, 0)); const int rc = reads_stage(st); if (rc) return rc; }
            // the second pass (overflow list of the first; global tables beyond) has usually nothing to do and is queued all the
            // same: whether it has is known when the first pass ends, and nothing is carried over from earlier runs
            const int gt_grid = O.gt_grid > 0 ? O.gt_grid : GT_GRID;
            if (B.r_start.p32) {
                hipLaunchKernelGGL((k_genotype<1024, 4, false, true>), dim3(gt_grid), dim3(256), 0, st, B);
                hipLaunchKernelGGL((k_genotype<8192, 4, true, true>), dim3(256), dim3(256), 0, st, B);
            } else {
                hipLaunchKernelGGL((k_genotype<1024, 4, false, false>), dim3(gt_grid), dim3(256), 0, st, B);
                hipLaunchKernelGGL((k_genotype<8192, 4, true, false>), dim3(256), dim3(256), 0, st, B);
            }
#ifdef CSV_GT_PROF
            hipLaunchKernelGGL(k_gt_prof_print, dim3(1), dim3(1), 0, st, B);
#endif
            DBG("genotype");
            HIP_TRY(c, mark());
        } else if (stats) { for (int q = 0; q < 4; q++) HIP_TRY(c, mark()); }
        if (c->bt.any_tra_gt) {
            // (reads_off / contig_len / the reads columns travel on side[2]: a batch whose only genotyped segments are TRA
            // segments, or one without reads, has not waited for them yet)
            if (c->bt.copies_pending && c->ro.have_tab) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_reads, 0));
            if (B.r_start.p32) LAUNCH("genotype_tra", k_genotype_tra<true>, 256, 64, 0, B);
            else LAUNCH("genotype_tra", k_genotype_tra<false>, 256, 64, 0, B);
        } else HIP_TRY(c, mark());
        // one more record with nothing in front of it: what a slot reads when it holds no kernel (the event records occupy the
        // stream themselves).  bench.py subtracts THIS from the kernel slots instead of guessing an empty one.
        HIP_TRY(c, mark());
    }
#undef LAUNCH
#undef LAUNCH_ON
    if (c->bt.copies_pending) {
        // whatever this run did not consume is still waited for before the call returns (an empty batch; a reads table next
        // to zero signatures): the caller's page-locked columns must not be the source of a copy in flight after the call,
        // and the next upload re-plans the arena
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_copy[1], 0));
        if (c->ro.have_tab) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_reads, 0));
        c->bt.copies_pending = false;
    }
    HIP_TRY(c, hipGetLastError());
    c->bt.ran = true;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        const int rc = read_counters(c);
        if (rc) return rc;
        for (int i = 0; i + 1 < ev && i < CSV_N_STAGES; i++) HIP_TRY(c, hipEventElapsedTime(&stats->ms_stage[i], c->ev[i], c->ev[i + 1]));
        HIP_TRY(c, hipEventElapsedTime(&stats->ms_total, c->ev[0], c->ev[ev - 1]));
        stats->n_clusters = c->res.h_cnt.n_clusters;
        stats->n_work_block = c->res.h_cnt.n_items_big;
        stats->n_work_wave = c->res.h_cnt.n_items - c->res.h_cnt.n_items_big;
        stats->n_calls = c->res.h_cnt.n_calls;
        stats->n_support = c->res.h_cnt.n_support;
    }
    return CSV_OK;
}

// device counters -> c->res.h_cnt (through the page-locked block).  A reads table that the run-level reorder could not
// handle switches the batch to the general sort and runs it again, once.
int read_counters(csv_ctx* c)
{
    hipStream_t st = c->stream;
    for (int attempt = 0; attempt < 2; attempt++) {
        HIP_TRY(c, hipMemcpyAsync(c->h_pin, c->bt.B.cnt, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        memcpy(&c->res.h_cnt, c->h_pin, sizeof(DevCounters));
        {   // the reads-order state of the upload lives outside the per-run counters
            ReadsState rs{};
            HIP_TRY(c, hipMemcpy(&rs, c->ro.rstate.p, sizeof rs, hipMemcpyDeviceToHost));
            c->res.h_cnt.n_runs = rs.n_runs; c->res.h_cnt.ro_state = rs.ro_state; c->res.h_cnt.error |= rs.error;
        }
        if (c->opt.debug_counters)
            fprintf(stderr, "[csv] counters: clusters %d items %d calls %d error %d | reads: mode %d runs %d state %d | gt_over %d gt_huge %d tra_huge %d\n",
                    c->res.h_cnt.n_clusters, c->res.h_cnt.n_items, c->res.h_cnt.n_calls, c->res.h_cnt.error, c->bt.B.ro_mode, c->res.h_cnt.n_runs, c->res.h_cnt.ro_state,
                    c->res.h_cnt.n_gt_over, c->res.h_cnt.n_gt_huge, c->res.h_cnt.n_tra_huge);
        if (c->bt.B.ro_mode == 1 && c->bt.B.n_reads > 0 && c->bt.any_genotype && c->res.h_cnt.ro_state == RO_NEED_GENERAL && attempt == 0) {
            c->ro.reads_general = true;
            c->bt.B.ro_mode = 2;
            c->ro.reads_ready = false;
            const int rc = run_impl(c, nullptr);
            if (rc) return rc;
            continue;
        }
        break;
    }
    return CSV_OK;
}

}  // namespace

extern "C" {

int csv_batch_run(csv_ctx* c, csv_run_stats* stats)
{
    if (!c) return CSV_E_INVALID;
    if (!c->bt.uploaded) return fail(c, CSV_E_STATE, "csv_batch_run before csv_batch_upload");
    return run_impl(c, stats);
}

int csv_batch_validate(csv_ctx* c)
{
    if (!c) return CSV_E_INVALID;
    if (!c->bt.uploaded) return fail(c, CSV_E_STATE, "csv_batch_validate before csv_batch_upload");
    if (c->bt.partial_cols) return fail(c, CSV_E_STATE, "csv_batch_validate needs a csv_batch_upload: a csv_cluster_batch call from page-locked columns keeps only the rows its kernels read");
    if (c->res.n_pend) return fail(c, CSV_E_STATE, "csv_batch_validate while %d asynchronous publish(es) are in flight: csv_batch_publish_wait first", c->res.n_pend);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // k_validate_order reports through the batch's counter pointer.  That pointer alternates between the two result arenas
    // from run to run (advisor, r05: clearing and reading arena 0 while the kernel wrote arena 1 returned CSV_OK for an
    // unsorted batch after an odd number of runs): the check gets a counter block of its own, which no run and no publish uses.
    DevBatch V = c->bt.B;
    V.cnt = (DevCounters*)((char*)c->res.cnt.p + 512);
    HIP_TRY(c, hipMemsetAsync(V.cnt, 0, sizeof(DevCounters), st));
    if (V.W > 0) hipLaunchKernelGGL(k_validate_order, dim3(div_up(V.W, 256)), dim3(256), 0, st, V);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->h_pin, V.cnt, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    memcpy(&c->res.h_cnt, c->h_pin, sizeof(DevCounters));
    c->bt.ran = false;
    if (c->res.h_cnt.error & ERR_SIG_ORDER)
        return fail(c, CSV_E_UNSORTED, "a segment is not in the rebuild order of cuteSV (main script :764-802) or holds adjacent duplicates");
    return CSV_OK;
}

int csv_cluster_batch(csv_ctx* c, const csv_batch_in* in, csv_batch_out* out)
{
    if (!c || !in || !out) return CSV_E_INVALID;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    int rc = upload_impl(c, in, out->cluster_id != nullptr || out->allele_id != nullptr, false, true);
    const bool tm = c->opt.debug_timing;                    // (CSV_DEBUG_TIMING, as the upload just read it)
    const double t1 = tm ? now() : 0;
    if (rc == CSV_OK) rc = run_impl(c, nullptr);
    const double t2 = tm ? now() : 0;
    if (tm && rc == CSV_OK) { (void)hipStreamSynchronize(c->stream); }
    const double t3 = tm ? now() : 0;
    if (rc == CSV_OK) rc = csv_batch_download(c, out);
    if (tm) fprintf(stderr, "[csv] one shot: upload issue %.3f ms, run issue %.3f ms, wait for the kernels %.3f ms, download %.3f ms, total %.3f ms\n",
                    t1 - t0, t2 - t1, t3 - t2, now() - t3, now() - t0);
    // the caller's columns may still be the source of a copy in flight when something failed on the way
    if (rc != CSV_OK && rc != CSV_E_CAPACITY) (void)hipDeviceSynchronize();
    return rc;
}

}  // extern "C"
