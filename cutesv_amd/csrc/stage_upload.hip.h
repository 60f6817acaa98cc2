// stage_upload.hip.h — engine, host -> device: csv_batch_upload and the upload half of csv_cluster_batch.  upload_impl is a list of
// phases over one UploadPlan; the environment is read here (load_run_opts) and nowhere else in the engine.  State: BatchState,
// ReadsOrderState, TableState (ctx.hip.h).  Host code only.
namespace {

int env_int(const char* name, int dflt)
{
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

void load_run_opts(csv_ctx* c)
{
    auto& o = c->opt;
    o.debug = getenv("CSV_DEBUG") != nullptr;
    o.debug_counters = o.debug || getenv("CSV_DEBUG_COUNTERS") != nullptr;
    o.debug_timing = getenv("CSV_DEBUG_TIMING") != nullptr;
    o.no_fork = getenv("CSV_NO_FORK") != nullptr;
    o.fork_always = getenv("CSV_FORK_ALWAYS") != nullptr;
    o.no_swap = getenv("CSV_NO_SWAP") != nullptr;
    o.no_peek = getenv("CSV_NO_PEEK") != nullptr;
    o.no_pair_in_mid = getenv("CSV_NO_PAIR_IN_MID") != nullptr;
    o.no_publish = getenv("CSV_NO_PUBLISH") != nullptr;
    o.iw_grid = env_int("CSV_IW_GRID", 0);
    o.gt_grid = env_int("CSV_GT_GRID", 0);
    o.tier_fork_min = env_int("CSV_TIER_FORK_MIN", 1 << 30);
    o.mid_grid = env_int("CSV_MID_GRID", 0);
    o.big_grid = env_int("CSV_BIG_GRID", 0);
    o.pub_inplace = getenv("CSV_PUB_INPLACE") != nullptr;
    o.no_reads_overlap = getenv("CSV_NO_READS_OVERLAP") != nullptr;
    o.no_lazy = getenv("CSV_NO_LAZY") != nullptr;
    o.lazy_min = env_int("CSV_LAZY_MIN", 64 << 10);
    o.no_rows8 = getenv("CSV_NO_ROWS8") != nullptr;
    o.no_delta16 = getenv("CSV_NO_DELTA16") != nullptr;
    o.delta16_min = env_int("CSV_DELTA16_MIN", 32 << 10);
    o.delta16_esc = env_int("CSV_DELTA16_ESC", 64);
    o.copy_stream = env_int("CSV_COPY_STREAM", 0) != 0;
    o.no_tiny = getenv("CSV_NO_TINY") != nullptr;
    o.reads_gap = env_int("CSV_READS_GAP", 1000000);
}

// `num ** 0.5` of cal_CIPOS is libm pow(), not sqrt() (GT:59; the two differ for 271 integers below 300 000): the device reads
// a table built with the host libm that covers every n an allele of the batch can have (n <= its segment's length).  Grown,
// never shrunk; a batch whose longest segment fits the table costs nothing here.
int sqrt_table(csv_ctx* c, i64 n)
{
    auto& T = c->tab;
    if (n <= T.sqrt_n) return CSV_OK;
    const i64 want = n + n / 4;
    std::vector<double> tab((size_t)want), rcp((size_t)want);
    std::vector<float> cipk((size_t)want);
    for (i64 i = 0; i < want; i++) {
        tab[(size_t)i] = pow((double)i, 0.5);
        rcp[(size_t)i] = i ? 1.0 / (double)i : 0.0;                                   // IEEE division: correctly rounded
        cipk[(size_t)i] = i ? (float)(1.96 / ((double)i * tab[(size_t)i])) : 0.0f;
    }
    HIP_TRY(c, hipDeviceSynchronize());                       // (a kernel of an earlier batch may still read the old tables)
    Buf* tb[3] = {&T.sqrt_tab, &T.rcp_tab, &T.cipk_tab};
    const void* src[3] = {tab.data(), rcp.data(), cipk.data()};
    const size_t esz[3] = {sizeof(double), sizeof(double), sizeof(float)};
    for (int q = 0; q < 3; q++) {
        if (tb[q]->p) { HIP_TRY(c, hipFree(tb[q]->p)); tb[q]->p = nullptr; tb[q]->cap = 0; }
        const int rc = reserve(c, *tb[q], (size_t)want * esz[q]);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpy(tb[q]->p, src[q], (size_t)want * esz[q], hipMemcpyHostToDevice));
    }
    T.sqrt_n = want;
    return CSV_OK;
}

// What an upload decides before it queues anything, on the stack of upload_impl: the phases below hand their results on through
// it and share no other local.  (Its two vectors are the ones the function always had.)
struct UploadPlan {
    // how the upload was asked for
    bool per_sig_forced = false, sync = true, lazy_ok = false;
    // sizes: segments, signatures in w space, reads, chain tiles, tiles of the reads table
    int  S = 0;
    i64  W = 0, R = 0, nt = 0, r_ntile = 0;
    // capacities: work items, temp calls, ints of the global hash pool
    i64  cap_items = 16, cap_tmp = 16, pool_n = 1 << 20;
    std::vector<uint8_t> drop;                              // per segment: genotyped, but its chromosome has no reads block
    // the forms
    bool per_sig = false, dev_cols = false, sig32 = false, rd32 = false;
    bool lazy = false;                                      // gate-first; the device addresses of the caller's page-locked columns:
    const void *lz_b = nullptr, *lz_rid = nullptr, *lz_aux = nullptr, *lz_rows8 = nullptr;
    bool delta16 = false;
    std::vector<std::pair<i64, int>> by_begin;              // (delta16) non-empty segments by their first source row
    bool r_gaps = false, r_lens = false, r_packed = false, r_overlap = false, reorder = false, have_tab = false;
    hipMemcpyKind col_kind = hipMemcpyHostToDevice, rd_kind = hipMemcpyHostToDevice;
    i64  n_anc_cap = 0, r_anc_cap = 0;                      // anchor capacities of the position column / the reads start column
    hipStream_t cs = nullptr;                               // the stream of the column copies
    // the staging block (page-locked) and, up to o_end, the small tables on the device: offsets and sizes
    size_t o_seg = 0, o_woff = 0, o_drop = 0, o_gate = 0, o_serr = 0, o_tiles = 0, o_end = 0, o_ones = 0, ones_bytes = 0, o_anc = 0, anc_bytes = 0,
           o_ranc = 0, ranc_bytes = 0, o_lesc = 0, lesc_bytes = 0, o_stage_end = 0;
};

// Phase 1, check and size: the header, the reads frame and every segment; h_seg, h_woff, the drop marks, the capacities and the
// any_* flags; the libm tables.  Queues nothing (it waits for publishes nobody waited for, and sqrt_table for the device when it grows).
int upload_check(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    auto& b = c->bt;
    if (c->res.n_pend) { (void)hipStreamSynchronize(c->res.pub); c->res.n_pend = 0; c->res.pend[0].live = c->res.pend[1].live = false; }      // (results nobody waited for)
    b.uploaded = b.ran = false; c->res.settled = false; c->res.parity = 0;
    b.lazy_pending = b.partial_cols = false; b.lazy_bytes = 0;
    c->ro.reads_general = false;
    c->ro.reads_ready = false;
    b.upload_seq0 = c->run_seq;
    load_run_opts(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (in->n_seg < 0 || in->n_sig < 0 || (in->n_seg > 0 && !in->seg)) return fail(c, CSV_E_INVALID, "bad batch header");
    // (support lists and seq_pick name signatures by their global index in 32 bits on the device)
    if (in->n_sig >= (1ll << 31)) return fail(c, CSV_E_INVALID, "n_sig = %lld: a batch indexes at most 2^31 - 1 signature rows (split the store)", (long long)in->n_sig);
    // CSV_IN_READS_DEVICE: the plain int32 columns only - the 16-bit and packed forms read r_start on the host (reads_anchors)
    const bool rd_dev = (in->flags & CSV_IN_READS_DEVICE) != 0;
    if (rd_dev && (!(in->flags & CSV_IN_READS_I32) || (in->flags & CSV_IN_READS_DELTA16) || in->r_delta || in->r_len16 || in->r_idp))
        return fail(c, CSV_E_INVALID, "CSV_IN_READS_DEVICE needs CSV_IN_READS_I32 and takes no r_delta / r_len16 / r_idp");
    U.rd_kind = rd_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;      // (reads_off and contig_len stay host arrays)
    const int S = U.S = in->n_seg;
    b.h_seg.assign(in->seg, in->seg + S);
    b.h_woff.assign(S + 1, 0);
    b.any_genotype = false;
    b.any_pair = false;
    b.any_tra_gt = false;
    const bool have_reads_off = in->reads_off != nullptr;
    if (have_reads_off) {                                   // the reads table is trusted by the kernels: check its frame here
        if (in->n_chrom < 0 || in->n_reads < 0 || in->n_reads >= (1ll << 31) - 4096) return fail(c, CSV_E_INVALID, "bad reads table header");
        if (in->reads_off[0] < 0) return fail(c, CSV_E_INVALID, "reads_off[0] is negative");
        for (int k = 0; k < in->n_chrom; k++)
            if (in->reads_off[k + 1] < in->reads_off[k]) return fail(c, CSV_E_INVALID, "reads_off decreases at chromosome %d", k);
        if (in->reads_off[in->n_chrom] > in->n_reads) return fail(c, CSV_E_INVALID, "reads_off[n_chrom] exceeds n_reads");
    }
    U.drop.assign(S + 1, 0);
    i64 cap_items = 16, cap_tmp = 16, maxseg_gt = 0, tra_gt_len = 0;
    for (int k = 0; k < S; k++) {
        const csv_segment& g = b.h_seg[k];
        if (g.svtype < CSV_DEL || g.svtype > CSV_TRA) return fail(c, CSV_E_INVALID, "segment %d: unknown svtype %d", k, g.svtype);
        if (g.sig_begin < 0 || g.sig_begin > g.sig_end || g.sig_end > in->n_sig) return fail(c, CSV_E_INVALID, "segment %d: bad signature range", k);
        if (g.genotype) {
            b.any_genotype = true;
            if (g.chrom < 0 || g.chrom >= in->n_chrom) return fail(c, CSV_E_INVALID, "segment %d: chrom %d outside the reads table", k, g.chrom);
            if (g.svtype == CSV_TRA) {
                // call_gt of cuteSV_resolveTRA.py:258-309 over the reads table; no "no reads block" gate there
                if (!in->reads_off || !in->contig_len) return fail(c, CSV_E_INVALID, "segment %d: TRA genotyping needs reads_off and contig_len", k);
                b.any_tra_gt = true;
            } else {
                U.drop[k] = (!in->reads_off || in->reads_off[g.chrom + 1] == in->reads_off[g.chrom]) ? 1 : 0;
            }
        }
        const i64 len = g.sig_end - g.sig_begin;
        if (g.genotype && g.svtype == CSV_TRA && len > tra_gt_len) tra_gt_len = len;
        if (g.genotype && g.svtype != CSV_TRA && len > maxseg_gt) maxseg_gt = len;
        if (len > 0 && g.svtype != CSV_DEL && g.svtype != CSV_INS) b.any_pair = true;
        b.h_woff[k + 1] = b.h_woff[k] + len;
        const i64 rc = g.read_count > 1 ? g.read_count : 1;
        const i64 msr = g.min_support_reads > 1 ? g.min_support_reads : 1;
        cap_items += len / rc + 1;
        if (g.svtype == CSV_DEL || g.svtype == CSV_INS) cap_tmp += len / msr + 1;
        else if (g.svtype == CSV_TRA) cap_tmp += 2 * (len / rc) + 2;
        else cap_tmp += len / rc + 1;
    }
    U.cap_items = cap_items; U.cap_tmp = cap_tmp;
    const i64 W = U.W = b.h_woff[S];
    {
        i64 longest = 0;
        for (int k = 0; k < S; k++) if (b.h_woff[k + 1] - b.h_woff[k] > longest) longest = b.h_woff[k + 1] - b.h_woff[k];
        const int rc = sqrt_table(c, longest + 2);
        if (rc) return rc;
    }
    if (W >= (1ll << 31) - 4096 || cap_tmp >= (1ll << 31) - 1) return fail(c, CSV_E_INVALID, "batch too large for 32-bit work indices (%lld signatures)", (long long)W);
    if (b.any_genotype && in->reads_off && (!in->r_start || !in->r_end || !in->r_primary || !in->r_id) && in->n_reads > 0)
        return fail(c, CSV_E_INVALID, "reads columns missing");
    const i64 R = U.R = (b.any_genotype && in->reads_off) ? in->n_reads : 0;
    U.have_tab = b.any_genotype && in->reads_off;
    U.nt = div_up(W, CH_TILE) + 2;                         // chain tiles
    U.r_ntile = div_up(R, CH_TILE);
    i64 rc_max = 0;                                        // largest reads block: bounds the cover set of one call
    if (R > 0) for (int k = 0; k < in->n_chrom; k++) { const i64 d = in->reads_off[k + 1] - in->reads_off[k]; if (d > rc_max) rc_max = d; }
    // global hash pool (ints, a power of two): holds the set of ANY call of the batch - supports <= its segment, cover <= two
    // scans of a reads block (genotype_global: table < 4 * need), TRA: < 59 * supports + 1710 ints (tra_bits_for)
    i64 pool_n = 1 << 20;
    if (R > 0) while (pool_n < 2 * (2 * rc_max + maxseg_gt) + 4096 || pool_n < 64 * tra_gt_len + 8192) { pool_n <<= 1; if (pool_n >= (1ll << 32)) break; }
    U.pool_n = pool_n;
    return CSV_OK;
}

// Phase 2, choose forms: gate-first, the position column as gaps (with the disjoint-segments test), the forms of the reads table.
// Queues nothing.
void upload_forms(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    auto& b = c->bt;
    const auto& O = c->opt;
    const int S = U.S;
    const i64 W = U.W, R = U.R;
    U.per_sig = U.per_sig_forced || (in->flags & CSV_IN_PER_SIG);
    U.dev_cols = (in->flags & CSV_IN_DEVICE_COLUMNS) != 0;       // a / b / read_id / aux are device pointers: device-to-device copies
    U.col_kind = U.dev_cols ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    U.sig32 = (in->flags & CSV_IN_SIG_I32) != 0; U.rd32 = (in->flags & CSV_IN_READS_I32) != 0;
    // Gate-first (one-shot calls only: the caller's columns are valid until the call returns): when b / read_id / aux live in
    // page-locked memory the device can read, only the position column travels in bulk and k_lazy_fetch pulls the rows of the
    // clusters that pass the size gate (kernels.hip.h).  Small batches are cheaper in one piece (CSV_LAZY_MIN signatures,
    // default 64 Ki: below that the extra kernel and its PCIe round trips cost more than the bytes they save).
    U.lazy = U.lazy_ok && !U.dev_cols && W > 0 && !O.no_lazy && W >= (i64)O.lazy_min && in->b && in->read_id && in->aux;
    if (U.lazy) {
        const size_t nb = (size_t)in->n_sig;
        // (ABI v8) {b, read_id} interleaved, page-locked: the fetch reads one array instead of two
        if (U.sig32 && in->rows8 && !O.no_rows8) U.lz_rows8 = pinned_device_address(in->rows8, nb * 8);
        if (!U.lz_rows8) {
            U.lz_b = pinned_device_address(in->b, nb * (U.sig32 ? 4 : 8));
            U.lz_rid = U.lz_b ? pinned_device_address(in->read_id, nb * 4) : nullptr;
        }
        U.lz_aux = (U.lz_rows8 || U.lz_rid) ? pinned_device_address(in->aux, nb * 4) : nullptr;
        U.lazy = U.lz_aux != nullptr;
    }

    // CSV_IN_SIG_DELTA16: the position column as 16-bit gaps + anchors (kernels.hip.h k_unpack_a16).  Needs disjoint segments (an
    // escape row belongs to one w): anything else takes the column itself.
    bool delta16 = U.sig32 && !U.dev_cols && W > 0 && (in->flags & CSV_IN_SIG_DELTA16) && in->a_delta && in->a && in->n_esc >= 0 &&
                   (in->n_esc == 0 || (in->a_esc_row && in->a_esc_val)) && !O.no_delta16 && W >= (i64)O.delta16_min &&
                   // a sparse column (sites far apart: a HiFi call set, the simulation beds) is mostly escapes: each costs the host an
                   // anchor (search + sort: 50 k of them 1.1 ms, measured on cfg4) and saves nothing - the column itself then
                   in->n_esc * (i64)O.delta16_esc <= in->n_sig;
    if (delta16) {
        for (int k = 0; k < S; k++) if (b.h_woff[k + 1] > b.h_woff[k]) U.by_begin.emplace_back(b.h_seg[k].sig_begin, k);
        std::sort(U.by_begin.begin(), U.by_begin.end());
        for (size_t i = 0; i + 1 < U.by_begin.size(); i++)
            if (b.h_seg[U.by_begin[i].second].sig_end > U.by_begin[i + 1].first) { delta16 = false; break; }
    }
    U.delta16 = delta16;
    U.n_anc_cap = delta16 ? (div_up(W, CH_TILE) + S + in->n_esc + 8) : 0;
    b.delta16 = delta16;

    U.reorder = R > 0 && !(in->flags & CSV_IN_READS_SORTED);
    // CSV_IN_READS_DELTA16: starts as gaps / ends as lengths, each only where escapes are rare (host work per escape, nothing saved)
    const bool rdz = U.rd32 && R > (i64)O.delta16_min && (in->flags & CSV_IN_READS_DELTA16) && !O.no_delta16;
    const i64 esc_per = (i64)O.delta16_esc;
    U.r_gaps = rdz && in->r_delta && in->r_start && in->n_r_esc >= 0 && (in->n_r_esc == 0 || (in->r_esc_row && in->r_esc_val)) && in->n_r_esc * esc_per <= R;
    U.r_lens = rdz && in->r_len16 && in->n_l_esc >= 0 && (in->n_l_esc == 0 || (in->l_esc_row && in->l_esc_val)) && in->n_l_esc * esc_per <= R;
    U.r_anc_cap = U.r_gaps ? (U.r_ntile + in->n_chrom + in->n_r_esc + 8) : 0;
    c->ro.reads_delta = (U.r_gaps ? 1 : 0) | (U.r_lens ? 2 : 0);
    c->ro.reads_early = false;
    U.r_packed = R > 0 && in->r_idp != nullptr && U.rd32 && !O.no_delta16;
    // all three 16-bit / packed forms on offer: the decode of one column runs (on a side stream, behind an event) while the next
    // column is on the link - id | primary first (the largest), the start gaps + their anchors, the lengths last, so that only
    // k_reads_end16 is left when the last byte has landed.  In one stream, in the order copies - copies - kernels, the three
    // decode kernels and the anchors' copy (95 us with their hand-overs) all followed the last byte.
    U.r_overlap = U.r_packed && U.r_gaps && U.r_lens && !O.no_reads_overlap;
}

// Phase 3, plan memory: one plan, one arena (it waits for the device only when the arena has to move); the small-table slices
// of `tabs`; room in the page-locked staging block.
int upload_memory(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    auto& b = c->bt;
    const int S = U.S;
    const i64 W = U.W, R = U.R, nt = U.nt, cap_items = U.cap_items, cap_tmp = U.cap_tmp;
    const i64 SC = 2 * W + 16 + 2 * ARR_PAD;
    // the small tables (segments, prefix, drop marks, gate records, status words, chain tile records) are ONE block laid out like
    // their page-locked staging copy: one DMA copy brings them all (r04: five blit kernels of ~5 us each in front of the columns)
    U.o_seg = 0; U.o_woff = U.o_seg + (size_t)(S + 1) * sizeof(csv_segment); U.o_drop = U.o_woff + (size_t)(S + 2) * 8;
    U.o_gate = (U.o_drop + (size_t)S + 1 + 15) & ~(size_t)15; U.o_serr = U.o_gate + (size_t)(S + 1) * 16;
    U.o_tiles = (U.o_serr + (size_t)(S + 1) * 4 + 15) & ~(size_t)15; U.o_end = U.o_tiles + (size_t)nt * TILE_REC * 16;
    U.o_ones = (U.o_end + 255) & ~(size_t)255; U.ones_bytes = (size_t)(CH_TILE + 64) * 8; U.o_anc = U.o_ones + U.ones_bytes;
    U.anc_bytes = U.delta16 ? (size_t)(div_up(W, CH_TILE) + 2 + 2 * U.n_anc_cap) * 4 : 0; U.o_ranc = U.o_anc + ((U.anc_bytes + 255) & ~(size_t)255);
    U.ranc_bytes = U.r_gaps ? (size_t)(U.r_ntile + 2 + 2 * U.r_anc_cap) * 4 : 0; U.o_lesc = U.o_ranc + ((U.ranc_bytes + 255) & ~(size_t)255);
    U.lesc_bytes = U.r_lens ? (size_t)(in->n_l_esc + 1) * 12 : 0; U.o_stage_end = U.o_lesc + ((U.lesc_bytes + 255) & ~(size_t)255);
    Plan P;
    P.add(b.tabs, U.o_end);
    // positions and lengths stay in the width they arrive in: the kernels read int32 columns as they are (kernels.hip.h Col)
    // (the position column is followed by a tile of padding, so that the chain kernel can read any span that begins inside the batch)
    if (U.sig32) { P.add(b.a32, (W + CH_TILE + 64) * 4); P.add(b.b32, (W + 1) * 4); } else { P.add(b.a, (W + CH_TILE + 64) * 8); P.add(b.b, (W + 1) * 8); }
    P.add(b.rid, (W + 1) * 4); P.add(b.aux, (W + 1) * 4);
    if (U.delta16) { P.add(b.ad16, (W + CH_TILE + 64) * 2); P.add(b.anc, (size_t)(div_up(W, CH_TILE) + 2 + 2 * U.n_anc_cap) * 4); }
    P.add(b.sup_tmp, (W + 1) * 4);
    if (U.per_sig) { P.add(b.cluster_id, (W + 1) * 4); P.add(b.allele_id, (W + 1) * 4); }
    P.add(b.partial, nt * 4); P.add(b.tile_cnt, nt * 16);
    if (U.lazy) P.add(b.tile_lead, nt * 4);
    if (U.per_sig) P.add(b.ch_masks, nt * CT_WORDS * 8);
    P.add(b.tile_items, nt * (size_t)TI_STRIDE * 16);
    P.add(b.item_rec, cap_items * 16); P.add(b.list_small, cap_items * 16); P.add(b.list_big, cap_items * 4); P.add(b.list_tiny, cap_items * 16); P.add(b.list_wide, cap_items * 16);
    P.add(b.item_cnt, cap_items * 8); P.add(b.item_base, (cap_items + 8) * 8); P.add(b.item_chunk, (cap_items / IS_CHUNK + 2) * 8);
    // temp call records are indexed by w (a cluster's slots live in its own signature range)
    P.add(b.t_rec, (W + 1) * sizeof(TmpRec)); P.add(b.t_rec0, (cap_items + 1) * sizeof(TmpRec));
    P.add(b.sc_k, SC * 8); P.add(b.sc_x, SC * 8); P.add(b.sc_v1, SC * 4); P.add(b.sc_v2, SC * 4); P.add(b.sc_v3, SC * 4); P.add(b.sc_v4, SC * 4); P.add(b.sc_v5, SC * 4);
    P.add(c->res.o_rec, (cap_tmp + 1) * sizeof(CallRec)); P.add(c->res.o_supsig, (W + 1) * 4); P.add(b.o_suprid, (W + 1) * 4);
    P.add(c->res.o_rec2, (cap_tmp + 1) * sizeof(CallRec)); P.add(c->res.o_supsig2, (W + 1) * 4);
    if (U.have_tab) { P.add(b.reads_off, (in->n_chrom + 1) * 8); P.add(b.contig_len, (in->n_chrom + 1) * 8); }
    if (R > 0) {
        P.add(b.gt_over, (cap_tmp + 2) * 4); P.add(b.gt_huge, (cap_tmp + 2) * 4); P.add(b.gt_pool, U.pool_n * 4);
        // the table as uploaded and its packed start-ordered form, both in the caller's width (int32: 13 + 12 bytes per read)
        const size_t cw = U.rd32 ? 4 : 8;
        P.add(b.r_start, R * cw); P.add(b.r_end, R * cw); P.add(b.r_primary, R); P.add(b.r_id, R * 4);
        if (U.r_gaps) { P.add(b.rd16, (R + CH_TILE + 64) * 2); P.add(b.ranc, (size_t)(U.r_ntile + 2 + 2 * U.r_anc_cap) * 4); }
        if (U.r_lens) { P.add(b.rl16, (R + 64) * 2); P.add(b.rlesc, (size_t)(in->n_l_esc + 1) * 12); }
        P.add(b.s_start, (R + 64) * cw); P.add(b.s_end, (R + 64) * cw); P.add(b.s_idp, (R + 64) * 4);      // (whole chunks of 64 rows are read)
        P.add(b.cmax, (div_up(R, 64) + 136) * 8); P.add(b.span_len, (div_up(R, 512) + 8) * 8); P.add(b.cfirst, (div_up(R, 64) + 136) * 8); P.add(b.bfirst, (div_up(R, 4096) + 136) * 8);      // (+ two steps of padding: k_genotype reads 128 entries from any valid one)
        P.add(b.maxlen, (in->n_chrom + 1) * 8);
        if (U.reorder) { P.add(c->ro.tcnt, (div_up(R, RO_TILE) + 1) * 4); P.add(c->ro.ent, (div_up(R, RO_TILE) + 1) * (size_t)RO_TCAP * 16); P.add(c->ro.tblk, (div_up(R, RO_TILE) + 2) * 4); P.add(c->ro.table, RO_CAP * 16); }
    }
    TRY(commit_synced(c, c->arena, P));
    {
        char* tb = (char*)b.tabs.p;
        b.seg.p = tb + U.o_seg; b.woff.p = tb + U.o_woff; b.seg_drop.p = tb + U.o_drop; b.seg_gate.p = tb + U.o_gate; b.seg_err.p = tb + U.o_serr; b.tile_info.p = tb + U.o_tiles;
    }
    // (the staging block is also the landing zone of the results: never smaller than one counters struct)
    return pin_reserve(c, U.o_stage_end + sizeof(DevCounters) + 256);
}

// Phase 4, the small tables: staged in page-locked memory, one copy on the main stream, behind the upload's fence (ev_init)
// and the zero fill of the reads-order state.
int upload_tables(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    (void)in;
    auto& b = c->bt;
    const int S = U.S;
    const i64 W = U.W, nt = U.nt;
    const std::vector<uint8_t>& drop = U.drop;
    hipStream_t st = c->stream;
    // The column copies go out on the kernels' OWN stream: the kernels that wait for them then wait on a barrier packet in
    // their queue.  On a copy stream of their own (r01-r04, CSV_COPY_STREAM=1) the dependency was an event across queues, which
    // this runtime resolves late: ~90 us between the end of the copy and the first kernel in a one-shot call (cfg3 gate-first
    // 0.64 -> 0.55 ms) - more than the chain kernels (~15 us) ever overlapped with the second copy group.
    U.cs = c->opt.copy_stream ? c->copy[0] : st;
    HIP_TRY(c, hipStreamSynchronize(st));                   // the staging block may still be the source of an earlier copy
    // whatever ran before (a resident caller's kernels still reading the columns this upload rewrites) is over before the
    // column copies start - and nothing else: they do not wait for the tables or the zero fills below
    HIP_TRY(c, hipEventRecord(c->ev_init, st));
    HIP_TRY(c, hipStreamWaitEvent(U.cs, c->ev_init, 0));
    memset(c->h_pin + U.o_serr, 0, (size_t)(S + 1) * 4);
    memcpy(c->h_pin + U.o_seg, b.h_seg.data(), (size_t)S * sizeof(csv_segment));
    memcpy(c->h_pin + U.o_woff, b.h_woff.data(), (size_t)(S + 1) * 8);
    memcpy(c->h_pin + U.o_drop, drop.data(), (size_t)S + 1);
    int* gate = (int*)(c->h_pin + U.o_gate);                // {read_count, dropped, svtype, -} per segment
    for (int k = 0; k < S; k++) { gate[4 * k] = b.h_seg[k].read_count; gate[4 * k + 1] = drop[k]; gate[4 * k + 2] = b.h_seg[k].svtype; gate[4 * k + 3] = 0; }
    {
        // per chain tile: first / last segment and the chain / gate scalars of up to three non-empty segments inline
        // (kernels.hip.h TILE_REC).  Empty segments own no row and are skipped.
        int* ti = (int*)(c->h_pin + U.o_tiles);
        memset(ti, 0, (size_t)nt * TILE_REC * 16);
        int k = 0;
        for (i64 t = 0; t < nt; t++) {
            int* r = ti + 4 * TILE_REC * t;
            const i64 w0 = t * (i64)CH_TILE, w1 = (w0 + CH_TILE < W ? w0 + CH_TILE : W) - 1;
            if (w0 >= W) { r[1] = -1; continue; }
            while (k + 1 < S && b.h_woff[k + 1] <= w0) k++;
            int k1 = k;
            while (k1 + 1 < S && b.h_woff[k1 + 1] <= w1) k1++;
            r[0] = k; r[1] = k1;
            int nin = 0;
            bool wide_bias = false;
            for (int q = k; q <= k1; q++) {
                if (b.h_woff[q + 1] == b.h_woff[q]) continue;
                if (nin < 3) {
                    const csv_segment& g = b.h_seg[q];
                    int* a = r + 4 + 4 * nin;
                    a[0] = (int)b.h_woff[q]; a[1] = g.read_count; a[2] = q | (g.svtype << 24) | (drop[q] ? (1 << 28) : 0); a[3] = (int)g.max_cluster_bias;
                    if (g.max_cluster_bias != (i64)(int)g.max_cluster_bias || q >= (1 << 24)) wide_bias = true;
                }
                nin++;
            }
            r[2] = (nin <= 3 && !wide_bias) ? nin : 0;
        }
    }
    // (the upload's reads-order state is cleared here, in FRONT of every copy - behind the column copies the fill kernel was one
    // more switch between the copy engine and the compute queue on the one-shot call's critical path - and only when there is a
    // reads table to order)
    if (U.have_tab || c->ro.rstate_dirty) { HIP_TRY(c, hipMemsetAsync(c->ro.rstate.p, 0, sizeof(ReadsState), st)); c->ro.rstate_dirty = U.have_tab; }
    HIP_TRY(c, hipMemcpyAsync(b.tabs.p, c->h_pin, U.o_end, hipMemcpyHostToDevice, st));
    return CSV_OK;
}

// The anchor tables of a column that crosses as 16-bit gaps (k_unpack_a16), for the position column (rows = w) and the reads
// start column alike: the collected {row, value} pairs sorted by row, one per row, written into the staging block at `dst` as
// {per-tile offsets [ntile + 2], rows [cap], values [cap]}.  Returns `dst` (the source of the copy).
int* stage_anchors(std::vector<std::pair<i64, int>>& anc, i64 ntile, i64 cap, char* dst)
{
    std::sort(anc.begin(), anc.end());
    anc.erase(std::unique(anc.begin(), anc.end(), [](const std::pair<i64, int>& x, const std::pair<i64, int>& y) { return x.first == y.first; }), anc.end());
    int* h_off = (int*)dst;
    int* h_w = h_off + ntile + 2;
    int* h_v = h_w + cap;
    size_t q = 0;
    for (i64 t = 0; t <= ntile; t++) {
        while (q < anc.size() && anc[q].first < t * (i64)CH_TILE) q++;
        h_off[t] = (int)q;
    }
    h_off[ntile + 1] = (int)anc.size();
    for (size_t i = 0; i < anc.size(); i++) { h_w[i] = (int)anc[i].first; h_v[i] = anc[i].second; }
    return h_off;
}

// Phase 5, the signature columns, on the copy stream U.cs (the main stream unless CSV_COPY_STREAM; the anchors of a delta16
// column on copy[0], the zero fills on the main stream), in two groups: what the chain kernels read (positions, lengths / pos2, the
// strand and chr2 words of INV / TRA segments), then what only the refine kernels read (read ids, INS sequence lengths).  In a
// one-shot call the chain kernels start when the first group has landed and run under the second.  Segments whose
// source ranges are adjacent travel as one copy; aux is not read for DEL / DUP segments (include/cutesv_hip.h) and is
// zero-filled on the device instead of crossing PCIe.  (One stream: a second DMA engine adds nothing on this link -
// scripts/micro/h2d_bw.hip measures 57 GB/s with 1, 2, 4 or 8 streams, from page-locked and pageable memory alike.)
// The padding behind the position column (positive values) is a DMA copy of a block of ones out of the staging area, in
// FRONT of the column: a fill kernel behind the DMA copy cost the stream an engine switch (~40 us in the trace) right
// where the chain kernels wait.
int upload_columns(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    auto& b = c->bt;
    const int S = U.S;
    const i64 W = U.W;
    const bool sig32 = U.sig32, delta16 = U.delta16, lazy = U.lazy;
    const hipMemcpyKind col_kind = U.col_kind;
    hipStream_t st = c->stream, cs = U.cs;
    {
        int* ones = (int*)(c->h_pin + U.o_ones);
        if (!delta16) for (size_t i = 0; i < U.ones_bytes / 4; i++) ones[i] = 1;
        if (delta16) {}                                   // (k_unpack_a16 writes the padding together with the column)
        else if (sig32) HIP_TRY(c, hipMemcpyAsync(dp<int>(b.a32) + W, ones, (size_t)(CH_TILE + 64) * 4, hipMemcpyHostToDevice, cs));
        else HIP_TRY(c, hipMemcpyAsync(dp<i64>(b.a) + W, ones, (size_t)(CH_TILE + 64) * 8, hipMemcpyHostToDevice, cs));
    }
    auto aux_kind = [&](int q) { const int t = b.h_seg[q].svtype; return t == CSV_INS ? 2 : (t == CSV_INV || t == CSV_TRA) ? 1 : 0; };
    for (int group = 1; group <= 2; group++) {
        for (int k = 0; k < S;) {
            int e = k;
            while (e + 1 < S && b.h_seg[e + 1].sig_begin == b.h_seg[e].sig_end) e++;
            const i64 src = b.h_seg[k].sig_begin, n = b.h_woff[e + 1] - b.h_woff[k], dst = b.h_woff[k];
            if (n > 0) {
                if (group == 1 && sig32) {
                    if (delta16) { HIP_TRY(c, hipMemcpyAsync(dp<uint16_t>(b.ad16) + dst, in->a_delta + src, n * 2, col_kind, cs)); b.lazy_bytes += n * 2; }
                    else HIP_TRY(c, hipMemcpyAsync(dp<int>(b.a32) + dst, (const int32_t*)in->a + src, n * 4, col_kind, cs));
                    if (!lazy) HIP_TRY(c, hipMemcpyAsync(dp<int>(b.b32) + dst, (const int32_t*)in->b + src, n * 4, col_kind, cs));
                } else if (group == 1) {
                    HIP_TRY(c, hipMemcpyAsync(dp<i64>(b.a) + dst, in->a + src, n * 8, col_kind, cs));
                    if (!lazy) HIP_TRY(c, hipMemcpyAsync(dp<i64>(b.b) + dst, in->b + src, n * 8, col_kind, cs));
                } else if (!lazy) HIP_TRY(c, hipMemcpyAsync(dp<int>(b.rid) + dst, in->read_id + src, n * 4, col_kind, cs));
                if (lazy && group == 2) b.lazy_bytes += n * (sig32 ? 4 : 8) + n * 4;      // b and read_id of the range stay behind
                for (int q = k; q <= e;) {                  // aux: runs of segments of this group's kind
                    int q2 = q;
                    while (q2 + 1 <= e && aux_kind(q2 + 1) == aux_kind(q)) q2++;
                    const i64 na = b.h_woff[q2 + 1] - b.h_woff[q];
                    if (aux_kind(q) == group && na > 0) {
                        if (!(lazy && group == 2)) HIP_TRY(c, hipMemcpyAsync(dp<int>(b.aux) + b.h_woff[q], in->aux + b.h_seg[q].sig_begin, na * 4, col_kind, cs));
                        else b.lazy_bytes += na * 4;
                    }
                    // aux of DEL / DUP segments is not the caller's to define (include/cutesv_hip.h): zero on the device.  Their own
                    // ranges only, on the main stream - nothing a copy writes, so the copies wait for no fill (gate-first: k_lazy_fetch
                    // writes the zeros of the rows it fetches)
                    if (group == 1 && aux_kind(q) == 0 && na > 0 && !lazy) HIP_TRY(c, hipMemsetAsync(dp<int>(b.aux) + b.h_woff[q], 0, (size_t)na * 4, st));
                    // gate-first: the chain predicates of INV / TRA segments read b (kernels.hip.h sig_flag): those ranges travel whole
                    if (lazy && group == 1 && aux_kind(q) == 1 && na > 0) {
                        const i64 sb = b.h_seg[q].sig_begin;
                        if (sig32) HIP_TRY(c, hipMemcpyAsync(dp<int>(b.b32) + b.h_woff[q], (const int32_t*)in->b + sb, na * 4, col_kind, cs));
                        else HIP_TRY(c, hipMemcpyAsync(dp<i64>(b.b) + b.h_woff[q], in->b + sb, na * 8, col_kind, cs));
                        b.lazy_bytes -= na * (sig32 ? 4 : 8);
                    }
                    q = q2 + 1;
                }
            }
            k = e + 1;
        }
        if (group == 1 && delta16) {
            // the anchors, built while the gaps are on the link: the first row of every chain tile, the first row of every
            // segment, the caller's escape rows that lie in a segment - {w, a[source row of w]} by ascending w, one slice per tile
            const int32_t* ha = (const int32_t*)in->a;
            const i64 ntile = div_up(W, CH_TILE);
            std::vector<std::pair<i64, int>> anc;
            anc.reserve((size_t)U.n_anc_cap);
            {
                int k = 0;
                for (i64 t = 0; t < ntile; t++) {
                    const i64 w = t * (i64)CH_TILE;
                    while (k + 1 < S && b.h_woff[k + 1] <= w) k++;
                    anc.emplace_back(w, ha[b.h_seg[k].sig_begin + (w - b.h_woff[k])]);
                }
            }
            for (auto& bk : U.by_begin) anc.emplace_back(b.h_woff[bk.second], ha[bk.first]);
            for (i64 e = 0; e < in->n_esc; e++) {
                const i64 g = in->a_esc_row[e];
                auto it = std::upper_bound(U.by_begin.begin(), U.by_begin.end(), std::make_pair(g, INT32_MAX));
                if (it == U.by_begin.begin()) continue;
                --it;
                const csv_segment& sg = b.h_seg[it->second];
                if (g >= sg.sig_end) continue;                      // (a row no segment of this batch holds)
                anc.emplace_back(b.h_woff[it->second] + (g - sg.sig_begin), in->a_esc_val[e]);
            }
            const int* h_off = stage_anchors(anc, ntile, U.n_anc_cap, c->h_pin + U.o_anc);
            // (on a copy stream of its own: behind the gaps on the kernels' stream it was 7 us of copy + 9 us of hand-over between
            // two copies on the call's critical path; here it lands while the gaps are still on the link, and the event has long
            // fired when k_unpack_a16 - queued behind the gaps - gets to wait for it)
            HIP_TRY(c, hipMemcpyAsync(b.anc.p, h_off, U.anc_bytes, hipMemcpyHostToDevice, c->copy[0]));
            HIP_TRY(c, hipEventRecord(c->ev_anc, c->copy[0]));
        }
        HIP_TRY(c, hipEventRecord(c->ev_copy[group - 1], cs));
    }
    b.copies_pending = true;                                // run_impl orders the kernels behind the two events
    return CSV_OK;
}

// anchors of the reads start column, built while the table is on the link: the first row of every tile of 2048 rows, the
// first row of every chromosome block, the caller's escape rows (the first row of every sorted run is one) - rows of
// the table itself: no w space here.  They follow the table on its own stream (page-locked staging: a copy out of pageable
// memory would block the host until the table in front of it on this stream has crossed the link).
int* reads_anchors(csv_ctx* c, const csv_batch_in* in, const UploadPlan& U)
{
    const i64 R = U.R;
    const int32_t* hs = (const int32_t*)in->r_start;
    std::vector<std::pair<i64, int>> anc;
    anc.reserve((size_t)U.r_anc_cap);
    for (i64 t = 0; t < U.r_ntile; t++) anc.emplace_back(t * (i64)CH_TILE, hs[t * (i64)CH_TILE]);
    for (int k = 0; k < in->n_chrom; k++) { const i64 r0 = in->reads_off[k]; if (r0 >= 0 && r0 < R) anc.emplace_back(r0, hs[r0]); }
    for (i64 e = 0; e < in->n_r_esc; e++) { const i64 r0 = in->r_esc_row[e]; if (r0 >= 0 && r0 < R) anc.emplace_back(r0, in->r_esc_val[e]); }
    return stage_anchors(anc, U.r_ntile, U.r_anc_cap, c->h_pin + U.o_ranc);
}

// the reads start column out of its gaps, on stream s
void reads_unpack(csv_ctx* c, const UploadPlan& U, hipStream_t s)
{
    auto& b = c->bt;
    const i64 r_ntile = U.r_ntile;
    UnpackArgs UA{dp<uint16_t>(b.rd16), dp<int>(b.r_start), U.R, dp<int>(b.ranc), dp<int>(b.ranc) + r_ntile + 2, dp<int>(b.ranc) + r_ntile + 2 + U.r_anc_cap, (int)r_ntile, 0, 0};
    DevBatch none;
    memset(&none, 0, sizeof none);
    hipLaunchKernelGGL(k_unpack_a16, dim3((unsigned)r_ntile), dim3(256), 0, s, UA, none);
}

// the reads end column out of the starts and the 16-bit lengths, then the caller's escape rows over it, on stream s
int reads_ends(csv_ctx* c, const csv_batch_in* in, const UploadPlan& U, hipStream_t s)
{
    auto& b = c->bt;
    const i64 R = U.R;
    hipLaunchKernelGGL(k_reads_end16, dim3(div_up(R, 256)), dim3(256), 0, s, (const int*)dp<int>(b.r_start), (const uint16_t*)dp<uint16_t>(b.rl16), dp<int>(b.r_end), R);
    if (in->n_l_esc > 0) {
        char* base = (char*)b.rlesc.p;
        char* hst = c->h_pin + U.o_lesc;                  // (through the page-locked staging, as above)
        memcpy(hst, in->l_esc_row, (size_t)in->n_l_esc * 8);
        memcpy(hst + (size_t)in->n_l_esc * 8, in->l_esc_val, (size_t)in->n_l_esc * 4);
        HIP_TRY(c, hipMemcpyAsync(base, hst, (size_t)in->n_l_esc * 12, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_scatter_rows_i32, dim3(div_up(in->n_l_esc, 256)), dim3(256), 0, s, (const i64*)base, (const int*)(base + (size_t)in->n_l_esc * 8), dp<int>(b.r_end), in->n_l_esc, R);
    }
    return CSV_OK;
}

// Phase 6, the reads table, on its own stream (side[2] runs the reads_order / prefix-max kernels behind it), in its plain, packed
// and overlapped forms; the overlapped form decodes on side[1] and sends its anchors on copy[1].  Ends with ev_reads.
int upload_reads(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    auto& b = c->bt;
    const i64 R = U.R;
    const bool rd32 = U.rd32, r_gaps = U.r_gaps, r_lens = U.r_lens, r_packed = U.r_packed;
    const hipMemcpyKind rd_kind = U.rd_kind;
    hipStream_t sr = c->side[2];
    if (U.have_tab) {
        HIP_TRY(c, hipStreamWaitEvent(sr, c->ev_init, 0));
        HIP_TRY(c, hipMemcpyAsync(b.reads_off.p, in->reads_off, (size_t)(in->n_chrom + 1) * 8, hipMemcpyHostToDevice, sr));
        if (b.any_tra_gt && in->n_chrom > 0) HIP_TRY(c, hipMemcpyAsync(b.contig_len.p, in->contig_len, (size_t)in->n_chrom * 8, hipMemcpyHostToDevice, sr));
    }
    if (R > 0 && U.reorder) {
        // which chromosome blocks begin inside every tile of RO_TILE rows: k_reads_runs leaves a descent AT a block start out of
        // its lists (k_reads_plan adds every block start anyway; a reference with hundreds of small contigs has dozens of them
        // per tile)
        const int ntl = div_up(R, RO_TILE);
        c->ro.h_tblk.assign((size_t)ntl + 1, 0);
        int k = 0;
        for (int t = 0; t <= ntl; t++) {
            while (k < in->n_chrom && in->reads_off[k] < (i64)t * RO_TILE) k++;
            c->ro.h_tblk[(size_t)t] = k;
        }
        HIP_TRY(c, hipMemcpyAsync(c->ro.tblk.p, c->ro.h_tblk.data(), ((size_t)ntl + 1) * 4, hipMemcpyHostToDevice, sr));
    }
    if (R > 0 && U.r_overlap) {
        hipStream_t sk = c->side[1];
        // (the packed word lands where the packed start-ordered table will be built - s_idp is not written before k_reads_gather)
        HIP_TRY(c, hipMemcpyAsync(b.s_idp.p, in->r_idp, (size_t)R * 4, hipMemcpyHostToDevice, sr));
        HIP_TRY(c, hipEventRecord(c->ev_rd[0], sr));
        HIP_TRY(c, hipMemcpyAsync(b.rd16.p, in->r_delta, (size_t)R * 2, hipMemcpyHostToDevice, sr));
        HIP_TRY(c, hipEventRecord(c->ev_rd[1], sr));
        HIP_TRY(c, hipMemcpyAsync(b.rl16.p, in->r_len16, (size_t)R * 2, hipMemcpyHostToDevice, sr));
        // (the anchors travel on another copy stream: between two columns in this one they cost the link 34 us of turn-arounds)
        int* h_off = reads_anchors(c, in, U);
        HIP_TRY(c, hipStreamWaitEvent(c->copy[1], c->ev_init, 0));
        HIP_TRY(c, hipMemcpyAsync(b.ranc.p, h_off, U.ranc_bytes, hipMemcpyHostToDevice, c->copy[1]));
        HIP_TRY(c, hipEventRecord(c->ev_rd[3], c->copy[1]));
        HIP_TRY(c, hipStreamWaitEvent(sk, c->ev_rd[0], 0));
        hipLaunchKernelGGL(k_reads_split_idp, dim3(div_up(R, 256)), dim3(256), 0, sk, (const unsigned*)b.s_idp.p, dp<int>(b.r_id), dp<uint8_t>(b.r_primary), R);
        HIP_TRY(c, hipStreamWaitEvent(sk, c->ev_rd[1], 0));
        HIP_TRY(c, hipStreamWaitEvent(sk, c->ev_rd[3], 0));
        reads_unpack(c, U, sk);
        HIP_TRY(c, hipEventRecord(c->ev_rd[2], sk));
        HIP_TRY(c, hipStreamWaitEvent(sr, c->ev_rd[2], 0));          // (long fired when the lengths have crossed)
        TRY(reads_ends(c, in, U, sr));
        c->ro.reads_delta |= 4;
        c->ro.reads_early = true;                           // (the first run may order the table on the decode stream)
    } else if (R > 0) {
        const size_t cw = rd32 ? 4 : 8;
        if (r_gaps) HIP_TRY(c, hipMemcpyAsync(b.rd16.p, in->r_delta, (size_t)R * 2, hipMemcpyHostToDevice, sr));
        else HIP_TRY(c, hipMemcpyAsync(b.r_start.p, in->r_start, R * cw, rd_kind, sr));
        if (r_lens) HIP_TRY(c, hipMemcpyAsync(b.rl16.p, in->r_len16, (size_t)R * 2, hipMemcpyHostToDevice, sr));
        else HIP_TRY(c, hipMemcpyAsync(b.r_end.p, in->r_end, R * cw, rd_kind, sr));
        if (r_packed) {
            // (the packed word lands where the packed start-ordered table will be built - s_idp is not written before k_reads_gather -
            // and is split into the two columns the reads stage reads)
            HIP_TRY(c, hipMemcpyAsync(b.s_idp.p, in->r_idp, (size_t)R * 4, hipMemcpyHostToDevice, sr));
            hipLaunchKernelGGL(k_reads_split_idp, dim3(div_up(R, 256)), dim3(256), 0, sr, (const unsigned*)b.s_idp.p, dp<int>(b.r_id), dp<uint8_t>(b.r_primary), R);
            c->ro.reads_delta |= 4;
        } else {
            HIP_TRY(c, hipMemcpyAsync(b.r_primary.p, in->r_primary, R, rd_kind, sr));
            HIP_TRY(c, hipMemcpyAsync(b.r_id.p, in->r_id, R * 4, rd_kind, sr));
        }
        if (r_gaps) {
            int* h_off = reads_anchors(c, in, U);
            HIP_TRY(c, hipMemcpyAsync(b.ranc.p, h_off, U.ranc_bytes, hipMemcpyHostToDevice, sr));
            reads_unpack(c, U, sr);
        }
        if (r_lens) TRY(reads_ends(c, in, U, sr));
    }
    // (the main stream does not wait for the reads table: the kernels that read it are ordered behind this event)
    if (U.have_tab) HIP_TRY(c, hipEventRecord(c->ev_reads, sr));
    return CSV_OK;
}

// Behind every copy: the position column out of its gaps, and - a resident upload - the wait for the three streams.
int upload_unpack_and_wait(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    (void)in;
    auto& b = c->bt;
    hipStream_t st = c->stream;
    b.unpack_pending = false;
    if (U.delta16) {
        // The position column out of its gaps (k_unpack_a16) is queued behind EVERY copy of the upload, as the first kernel of
        // the run (a resident upload: right here).  Measured on cfg4 (80 MB of reads table on its own stream): the kernel queued
        // between the column copies delayed the copies behind it until the reads table had left the copy engine (1.77 -> 2.82 ms);
        // queued from here in a one-shot call, after the last copy, the launch itself blocked the host for 1.1 ms.
        const i64 ntile = div_up(U.W, CH_TILE);
        b.unpack_args = UnpackArgs{dp<uint16_t>(b.ad16), dp<int>(b.a32), U.W, dp<int>(b.anc), dp<int>(b.anc) + ntile + 2, dp<int>(b.anc) + ntile + 2 + U.n_anc_cap, (int)ntile, 0, 1};
        b.unpack_tiles = (int)ntile;
        b.unpack_pending = true;
        if (U.sync) {
            HIP_TRY(c, hipStreamWaitEvent(st, c->ev_copy[0], 0));
            HIP_TRY(c, hipStreamWaitEvent(st, c->ev_anc, 0));
            DevBatch none;                                // (a resident upload is never gate-first: nothing of the batch is read)
            memset(&none, 0, sizeof none);
            hipLaunchKernelGGL(k_unpack_a16, dim3((unsigned)ntile + 1), dim3(256), 0, st, b.unpack_args, none);
            b.unpack_pending = false;
        }
    }
    c->ro.have_tab = U.have_tab;
    if (U.sync) {
        HIP_TRY(c, hipStreamSynchronize(st)); HIP_TRY(c, hipStreamSynchronize(U.cs));
        if (U.have_tab) HIP_TRY(c, hipStreamSynchronize(c->side[2]));
        b.copies_pending = false;
    }
    return CSV_OK;
}

// Phase 7, bind: the DevBatch every kernel of the run takes.  Queues nothing (device columns: two blocking 4 / 8 byte reads).
int upload_bind(csv_ctx* c, const csv_batch_in* in, UploadPlan& U)
{
    auto& b = c->bt;
    const int S = U.S;
    const i64 R = U.R;
    const bool sig32 = U.sig32, per_sig = U.per_sig;
    DevBatch& B = b.B;
    memset(&B, 0, sizeof B);
    B.n_seg = S; B.n_chrom = in->n_chrom; B.W = U.W;
    B.seg = dp<csv_segment>(b.seg); B.woff = dp<i64>(b.woff); B.seg_drop = dp<uint8_t>(b.seg_drop);
    if (sig32) { B.a = Col{nullptr, dp<int>(b.a32)}; B.b = Col{nullptr, dp<int>(b.b32)}; }
    else { B.a = Col{dp<i64>(b.a), nullptr}; B.b = Col{dp<i64>(b.b), nullptr}; }
    B.rid = dp<int>(b.rid); B.aux = dp<int>(b.aux);
    B.per_sig = per_sig ? 1 : 0;
    B.end_z = 0;                                            // is the batch's last signature a (0,0) element?  (the reference's sentinel rule, INDEL:62-64)
    for (int k = S - 1; k >= 0; k--)
        if (b.h_seg[k].sig_end > b.h_seg[k].sig_begin) {
            const i64 last = b.h_seg[k].sig_end - 1;
            if (U.dev_cols) {                               // (columns in device memory: the two values are fetched)
                i64 va = 0, vb = 0; int32_t wa = 0, wb = 0;
                if (sig32) { HIP_TRY(c, hipMemcpy(&wa, (const int32_t*)in->a + last, 4, hipMemcpyDeviceToHost)); HIP_TRY(c, hipMemcpy(&wb, (const int32_t*)in->b + last, 4, hipMemcpyDeviceToHost)); va = wa; vb = wb; }
                else { HIP_TRY(c, hipMemcpy(&va, in->a + last, 8, hipMemcpyDeviceToHost)); HIP_TRY(c, hipMemcpy(&vb, in->b + last, 8, hipMemcpyDeviceToHost)); }
                B.end_z = va == 0 && vb == 0;
            } else
                B.end_z = sig32 ? (((const int32_t*)in->a)[last] == 0 && ((const int32_t*)in->b)[last] == 0) : (in->a[last] == 0 && in->b[last] == 0);
            break;
        }
    B.cluster_id = per_sig ? dp<int>(b.cluster_id) : nullptr; B.allele_id = per_sig ? dp<int>(b.allele_id) : nullptr;
    B.partial = dp<int>(b.partial); B.tile_cnt = dp<int4>(b.tile_cnt);
    B.item_rec = dp<int4>(b.item_rec); B.list_small = dp<int4>(b.list_small); B.list_big = dp<int>(b.list_big); B.list_tiny = dp<int4>(b.list_tiny); B.list_wide = dp<int4>(b.list_wide);
    B.seg_gate = dp<int4>(b.seg_gate); B.tile_info = dp<int4>(b.tile_info);
    if (U.lazy) { B.h_b = U.lz_b; B.h_rid = (const int*)U.lz_rid; B.h_aux = (const int*)U.lz_aux; B.h_rows8 = (const int2*)U.lz_rows8; B.tile_lead = dp<int>(b.tile_lead); b.lazy_pending = b.partial_cols = true; }
    B.ch_masks = per_sig ? dp<u64>(b.ch_masks) : nullptr; B.tile_items = dp<int4>(b.tile_items);
    B.seg_err = dp<int>(b.seg_err);
    B.tiny_max = c->opt.no_tiny ? 0 : 16;                      // (timing aid: 0 sends every DEL/INS cluster of m <= 32 through the paired path)
    B.item_cnt = dp<i64>(b.item_cnt); B.item_base = dp<i64>(b.item_base); B.item_chunk = dp<i64>(b.item_chunk);
    B.sup_tmp = dp<int>(b.sup_tmp);
    B.t_rec = dp<TmpRec>(b.t_rec); B.t_rec0 = dp<TmpRec>(b.t_rec0);
    B.cap_tmp = (int)U.cap_tmp; B.cap_items = (int)U.cap_items;
    B.sc_k = dp<u64>(b.sc_k); B.sc_x = dp<i64>(b.sc_x); B.sc_v1 = dp<int>(b.sc_v1); B.sc_v2 = dp<int>(b.sc_v2); B.sc_v3 = dp<int>(b.sc_v3); B.sc_v4 = dp<int>(b.sc_v4); B.sc_v5 = dp<int>(b.sc_v5);
    B.o_rec = dp<CallRec>(c->res.o_rec); B.o_supsig = dp<int>(c->res.o_supsig); B.o_suprid = dp<int>(b.o_suprid);
    B.n_reads = R;
    if (U.have_tab) { B.reads_off = dp<i64>(b.reads_off); B.contig_len = dp<i64>(b.contig_len); }
    if (R > 0) {
        if (U.rd32) { B.r_start = Col{nullptr, dp<int>(b.r_start)}; B.r_end = Col{nullptr, dp<int>(b.r_end)}; B.s_start32 = dp<int>(b.s_start); B.s_end32 = dp<int>(b.s_end); }
        else { B.r_start = Col{dp<i64>(b.r_start), nullptr}; B.r_end = Col{dp<i64>(b.r_end), nullptr}; B.s_start64 = dp<i64>(b.s_start); B.s_end64 = dp<i64>(b.s_end); }
        B.r_primary = dp<uint8_t>(b.r_primary); B.r_id = dp<int>(b.r_id);
        B.s_idp = dp<int>(b.s_idp); B.cmax = dp<void>(b.cmax); B.span_len = dp<i64>(b.span_len); B.cfirst = dp<void>(b.cfirst); B.bfirst = dp<void>(b.bfirst); B.maxlen = dp<i64>(b.maxlen);
        B.gt_over = dp<int>(b.gt_over); B.gt_huge = dp<int>(b.gt_huge);
        B.gt_pool = dp<int>(b.gt_pool); B.gt_pool_n = U.pool_n;
        B.ro_mode = U.reorder ? 1 : 0;
        if (U.reorder) {
            B.ro_tcnt = dp<int>(c->ro.tcnt); B.ro_ent = dp<int4>(c->ro.ent); B.ro_tblk = dp<int>(c->ro.tblk); B.ro_table = dp<int4>(c->ro.table); B.ro_cap = RO_CAP;
            B.ro_gap = c->opt.reads_gap;                       // (CSV_READS_GAP: tests shrink it together with their task regions)
        }
    }
    B.sqrt_tab = dp<double>(c->tab.sqrt_tab); B.rcp_tab = dp<double>(c->tab.rcp_tab); B.cipk_tab = dp<float>(c->tab.cipk_tab); B.cnt = dp<DevCounters>(c->res.cnt); B.rs = dp<ReadsState>(c->ro.rstate);
    b.n_sig_host = in->n_sig;
    b.n_reads = R;
    b.uploaded = true;
    return CSV_OK;
}

// Host -> device.  The small tables travel as ONE copy out of the page-locked staging block; the columns go out on the
// kernels' own stream, the reads table on its own so that the clustering kernels never wait
// for it.  `sync` = false (csv_cluster_batch): nothing waits here, the kernels are ordered behind the copies by events
// and the final download synchronises before the call returns.
int upload_impl(csv_ctx* c, const csv_batch_in* in, bool per_sig_forced, bool sync, bool lazy_ok)
{
    if (!c || !in) return CSV_E_INVALID;
    UploadPlan U;
    U.per_sig_forced = per_sig_forced; U.sync = sync; U.lazy_ok = lazy_ok;
    TRY(upload_check(c, in, U));
    upload_forms(c, in, U);
    TRY(upload_memory(c, in, U));
    TRY(upload_tables(c, in, U));
    TRY(upload_columns(c, in, U));
    TRY(upload_reads(c, in, U));
    TRY(upload_unpack_and_wait(c, in, U));
    return upload_bind(c, in, U);
}

}  // namespace

extern "C" {

int csv_batch_upload(csv_ctx* c, const csv_batch_in* in) { return upload_impl(c, in, false, true, false); }

int csv_batch_reads_mode(const csv_ctx* c) { return (c && c->bt.uploaded && c->bt.n_reads > 0) ? c->bt.B.ro_mode : -1; }

int csv_batch_info(const csv_ctx* c, int which, int64_t* value)
{
    if (!c || !value) return CSV_E_INVALID;
    if (which == 0) *value = c->bt.partial_cols ? 1 : 0;
    else if (which == 1) *value = c->bt.lazy_bytes;
    else if (which == 2) *value = c->bt.delta16 ? 1 : 0;
    else if (which == 3) *value = c->ro.reads_delta;
    else return CSV_E_INVALID;
    return CSV_OK;
}

int csv_batch_option(csv_ctx* c, int option, int value)
{
    if (!c) return CSV_E_INVALID;
    if (option == CSV_OPT_REUSE_READS_ORDER) { c->ro.reuse_reads = value != 0; return CSV_OK; }
    return fail(c, CSV_E_INVALID, "unknown option %d", option);
}

}  // extern "C"
