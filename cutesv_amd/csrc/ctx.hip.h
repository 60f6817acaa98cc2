// ctx.hip.h — the context of libcutesv_hip.so: one state struct per stage, of the extraction side and of the engine, each with the
// rule that says how long its buffers live; csv_ctx itself, which holds them next to what every entry shares (device, streams, events,
// arenas, staging, options); and the host helpers every entry shares: buffers and arenas, error reporting, the copy / timing / sort
// skeleton of the extraction stages.  Host code only; included by cutesv_hip.hip behind the kernel headers (one translation unit).
namespace {

struct Buf { void* p = nullptr; size_t cap = 0; };      // a slice of an arena (or, for the few stand-alone buffers, its own allocation)

// One device allocation for everything a batch needs: the buffers are planned (sizes -> offsets), the arena grows
// only when the plan does not fit, and every Buf becomes a pointer into it.  (The first version reserved ~90 buffers
// with one hipMalloc each: 2.7 ms on the first upload, and a larger batch re-allocated them one by one.)
struct Arena { char* base = nullptr; size_t cap = 0; };
struct Plan {
    std::vector<std::pair<Buf*, size_t>> items;
    size_t total = 0;
    void add(Buf& b, size_t bytes)
    {
        items.emplace_back(&b, total);
        b.cap = bytes;
        total += (bytes + 255) & ~(size_t)255;
    }
};

// ---- The state of the extraction-side stages (stage_*.hip.h), one struct each, with the rule that says how long its buffers
// live and who may read them after the call returns.  `own` lists the stand-alone allocations for csv_ctx_destroy (slices
// of an arena go with their arena).

// The device-resident signature pool: stand-alone, grown by copying.  The rows live until csv_pool_reset; the CIGAR and
// split entries append to them (CSV_CG_TO_POOL), the rebuild reads them (CSV_RB_FROM_POOL).
struct PoolState {
    Buf seg, a, b, read, aux;
    i64 n = 0, cap = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&seg, &a, &b, &read, &aux}); }
};
// The device-resident name pool (names.hip.h): blob = the names back to back, off = n + 1 offsets into it (stand-alone, grown
// by copying), len = the lengths once more on the host (csv_name_pool_get sizes its blob from them).  rank / first hold the
// ranks of the first n names while `fresh`, until the next append or reset: the rebuild reads rank in place
// (CSV_RB_RANK_FROM_NAMES).  The sort's scratch is slices of `arena`, dead when the ranks are made.
struct NameState {
    Buf blob, off, rank, first, get;
    Arena arena;
    Buf words, perm0, perm1, hist, tot, vary, flag, partial;
    std::vector<uint8_t> len;
    i64 n = 0, bytes = 0, distinct = 0;
    bool fresh = false;
    float ms = 0; int passes = 0, maxlen = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&blob, &off, &rank, &first, &get}); }
};
// Rebuild, CIGAR scan and split analysis: slices of csv_ctx::scratch, which every call of the three plans afresh.  Dead when
// the call returns, with one exception: the caller of a CSV_RB_KEEP_ON_DEVICE rebuild may read oseg .. osrc (the dev_*
// pointers of csv_rebuild_out) until the next call of ANY of the three.  The rebuild counts into the engine's counter block
// (ResultState cnt + 768), so it clears the batch's `uploaded` and `ran`.  sp.qlen (the query lengths of a CSV_CG_TO_POOL call) stands alone.
struct RebuildState {
    Buf seg, a, b, rid, aux, auxk, major, nodedup, perm0, perm1, hist, tot, partial;
    Buf oseg, oa, ob, orid, oaux, osrc, segcnt, rank, mx, drop, el0, el1;
    int route = 0;          // csv_rebuild_route: the sort the last successful call took
};
struct CigarState { Buf qlen, off, ops, start, use, cnt, tiles, tot, iread, ipos, ilen, ip0, inp, pq, pl, dread, dpos, dlen; };
struct SplitState {
    Buf off, len, c0, c1, f0, f1, chr, mapq, strand, primary, seg, cnt, tiles, tot, kind, read, ochr, aux, a, b, c, d, qlen;
    void own(std::vector<Buf*>& v) { v.push_back(&qlen); }
};
// BAM decode: slices of `arena`; the SA ranges are sized after the scan, so they stand alone.  Everything lives until the next
// decode: csv_cigar_signatures with CSV_CG_FROM_BAM scans cigoff / cigar / start in place, csv_bam_split_inputs reads slim
// and the record columns, the caller the dev_* pointers of csv_bam_out.  gates (csv_bam_task_gates: a byte of CSV_GATE_* bits per
// record) and gtab (its region table, dead when that call returns) stand alone; the gates belong to the decode they were made
// from (gates_ok) and die with it: CSV_CG_USE_FROM_GATES and CSV_SA_SEL_FROM_GATES read them in place.
struct BamState {
    Arena arena;
    Buf slim, recoff, reclen, start, end, flag, mapq, qlen, cl, cr, cls, status, cigoff, saoff, cigsrc, cgb, cge, cigar, long_list, cnt, tot;
    Buf sabeg, saend, gates, gtab;
    i64 n = -1, nops = 0, nsa = 0;             // records / operations / SA tags of the last successful decode (-1: none)
    bool gates_ok = false;                     // `gates` holds the gates of that decode
    std::vector<i64> gtab_h;                   // the host image of gtab: the source of an asynchronous upload, so it lives here and not on a stack
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&sabeg, &saend, &gates, &gtab}); }
};
// Split inputs of the last decode (sa.hip.h): the tables sized before the kernels run are slices of `arena`, the entry columns
// are sized by the count pass and stand alone.  They live until the next decode or the next csv_bam_split_inputs:
// csv_split_signatures with CSV_SP_FROM_BAM reads them in place.
struct SaState {
    Arena arena;
    Buf sel, names, nameoff, namerank, calloff, callrec, callsa, entoff, readlen, status, tot;
    Buf c0, c1, f0, f1, chr, mapq, strand, primary;
    i64 calls = -1, entries = 0;               // calls / entries the context holds (-1: no split inputs)
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&c0, &c1, &f0, &f1, &chr, &mapq, &strand, &primary}); }
};
// The INS sequence pool (seqs.hip.h), in two parts, all stand-alone.  (1) The read sequences of the current batch: the packed
// 4-bit image csv_seq_reads_upload made, with per read its offset and length (-1: not uploaded), indexed by the batch's read
// index; they live until the next upload or the next csv_bam_decode (n_reads = -1: none).  qrev: the strand byte per read of a
// host-fed split analysis (csv_seq_query_reverse), dead with the upload.  (2) The shadow of the signature pool: blob = the ASCII
// bases back to back (grows only, by copying), off / half = per POOL ROW the first byte (-1: no sequence) and the x.5 flag; the
// row arrays grow with the pool (pool_reserve) and hold values for the rows [0, rows) - seq_sync fills up to the pool's count.
// They live until csv_pool_reset.  Per-call scratch, dead when the call returns: plan (lengths and their scan of an attach), tie (group tables and
// the answer of k_seq_tie_order), get (row / offset tables of put and get), out (the gathered bases of a get on their way to the host).
// whole: csv_seq_option(CSV_SEQ_OPT_WHOLE_IMAGE), the measurement aid.
struct SeqState {
    Buf rbytes, roff, rlen, qrev;
    i64 n_reads = -1, n_qrev = -1;
    Buf blob, off, half;
    i64 rows = 0, rows_cap = 0, bytes = 0, n_with = 0;
    Buf plan, tie, get, out;
    bool whole = false;
    csv_seq_info info{};
    i64 device_bytes() { std::vector<Buf*> v; own(v); i64 t = 0; for (Buf* b : v) t += (i64)b->cap; return t; }
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&rbytes, &roff, &rlen, &qrev, &blob, &off, &half, &plan, &tie, &get, &out}); }
};
// The VCF strings (vcf_strings.hip.h): csv_seq_alt_gather and csv_name_support_join read the sorted columns of the last KEPT pool
// rebuild (CSV_RB_FROM_POOL | CSV_RB_KEEP_ON_DEVICE: rb.osrc / orid / oaux, n_out rows) together with the pools those columns
// number.  gen counts the events after which they no longer belong together - a pool reset or append, a name-pool reset or
// append, any rebuild, any call that plans csv_ctx::scratch afresh; kept = gen when that rebuild finished (0: none): the two
// entries run only while kept == gen.  work (picks / supports, lengths, scan tables) and out (the blob on its way to the host)
// stand alone and are dead when a call returns.
struct VcfStrState {
    uint64_t gen = 1, kept = 0;
    i64 n_out = 0;
    bool by_name = false;
    Buf work, out;
    void stale() { gen++; }
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&work, &out}); }
};
// The alignment table (aln.hip.h): one row per BAM record - start, end, name id | primary << 31 - grouped by chromosome, in
// file order; all stand-alone.  start / end / idp grow by copying and hold n rows; maxlen = per chromosome the longest
// end - start, kept on the device (atomicMax as rows arrive); h_off = the row offsets per chromosome, kept on the host (it learns
// every append's count) and sent with the tables of a genotype call; last_chrom / max_id: the chromosome of the last row and the largest name id seen, for the
// host checks.  The rows live until csv_aln_reset.  Dead when a call returns: work (an append's flags, scan tables and pending
// words; a host append's columns), gt (the tables of a csv_aln_tra_genotype call, its results, the global sets of its large calls).
struct AlnState {
    Buf start, end, idp, maxlen, work, gt;
    std::vector<i64> h_off;
    i64 n = 0, max_id = -1;
    int n_chrom = 0, last_chrom = -1;
    float ms_append = 0, ms_genotype = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&start, &end, &idp, &maxlen, &work, &gt}); }
};
// The genotyping reads table (reads.hip.h): one row per gated record - start, end, primary, name id - grouped by chromosome, in
// append order; all stand-alone.  start / end / primary / id grow by copying and hold n rows; h_off = the row offsets per chromosome,
// kept on the host (it learns every append's count) and handed to the engine as reads_off; last_chrom / max_id: the chromosome of
// the last row and the largest name id seen, for the host checks; n_chrom = -1 until the first csv_reads_reset.  The rows live until
// csv_reads_reset.  Dead when a call returns: work (an append's keep bytes, scan tables and totals; a host append's columns).  rid
// (the rank column of a csv_reads_batch_columns call) lives until the next such call or reset: the engine copies it at upload.
struct ReadsTabState {
    Buf start, end, primary, id, work, rid;
    std::vector<i64> h_off;
    i64 n = 0, max_id = -1;
    int n_chrom = -1, last_chrom = -1;
    float ms_append = 0, ms_columns = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&start, &end, &primary, &id, &work, &rid}); }
};

// BGZF inflate (stage_inflate.hip.h): the payloads, the block tables, the inflated bytes and the status bytes of ONE csv_bgzf_inflate
// call, all stand-alone and grow-only; dead when the call returns.  No other stage reads or writes them, and the entry touches nothing
// else of the context but its stream and its first two timing events.  tab_h / order: the host image of the tables and the blocks in
// output order (the overlap check, the runs of the download).
struct InflateState {
    Buf comp, tab, out, status;
    std::vector<char> tab_h;
    std::vector<int32_t> order;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&comp, &tab, &out, &status}); }
};

// BGZF deflate (stage_deflate.hip.h): the input bytes, the block table, one 65536-byte slot per block, the token
// scratch of the grid's wavefronts, the sizes, the offsets and the packed file image of ONE csv_bgzf_deflate call.  Stand-alone and
// grow-only; dead when the call returns; no other stage reads or writes them.
struct DeflateState {
    Buf in, tab, slots, tok, size, offs, image;
    std::vector<char> tab_h;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&in, &tab, &slots, &tok, &size, &offs, &image}); }
};

// The VCF records (stage_vcf_emit.hip.h): work (the view's tables, the emission order, the three count columns, the
// scan's tile sums and totals), blobs (the REF, ALT and RNAMES bytes the caller sent), alt / rn (the ALT and RNAMES bytes gathered from a
// kept rebuild, CSV_VCF_*_FROM_POOL) and rows are dead when csv_vcf_emit_device returns.
// text - the prefix and the records behind it - is dead too unless the call asked for CSV_VCF_KEEP_TEXT: then text[0 .. text_bytes)
// stays, `kept` is set, and csv_vcf_text_fetch / csv_bgzf_deflate_text read it until the next csv_vcf_emit_device, which drops it
// (gen counts the emits: a caller's handle is good while the context's gen is its own).  Stand-alone and grow-only; no other stage
// reads or writes them.
struct VcfEmitState {
    Buf work, blobs, alt, rn, text, rows;
    uint64_t gen = 0;
    bool kept = false;
    i64 text_bytes = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&work, &blobs, &alt, &rn, &text, &rows}); }
};

// Reference gather (stage_ref.hip.h): the inflated bytes of the touched blocks, the block and range tables and
// the gathered bases of ONE csv_ref_gather call.  Stand-alone and grow-only; dead when the call returns; no other stage reads or
// writes them (the inflate in front of the gather runs through InflateState's buffers, which are as dead between calls).
struct RefState {
    Buf data, tab, out, fai, fai_rows;      // fai: k_fai_events' tile tables and its FaiOut
    std::vector<char> tab_h;
    std::vector<int64_t> data_off;
    std::vector<long long> out_off, tile_first;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&data, &tab, &out, &fai, &fai_rows}); }
};

// Record framing on the device (stage_frame.hip.h), all stand-alone and grow-only.  win: the two window
// buffers of the reader - win[cur] holds the inflated window [0, win_n), the other one receives the next window, whose kept tail is
// copied over from win[cur] (two buffers: no copy overlaps).  tab (block tables, guesses, exits, counts, the scan's work space, the
// stitch's verdict), starts, rows, pack: dead when a csv_frame_run / csv_frame_pack returns.  slim / host: the device images of the
// chunk the reader `owner` handed out last, with the host copies of its offset and length columns; they live until that reader's
// next read or route change (chunk_ok), and the *_framed consumers read them there (the decode copies the slim image device to
// device into BamState's arena, where the later stages expect it).  One reader frames on a context at a time (reader).  No other stage reads or writes any of
// this, and the entries touch nothing else of the context but its stream and its first four timing events.
struct FrameState {
    Buf win[2], tab, starts, rows, pack, slim, host, cols;
    int cur = 0;
    i64 win_n = 0;
    uint64_t serial = 0;                       // windows loaded so far (csv_frame_window_serial)
    std::vector<char> tab_h;
    std::vector<FrRow> rows_h;
    i64 n_rows = 0;                            // rows of the last csv_frame_run, in `rows` (device)
    const void* reader = nullptr;              // the one reader that frames on this context (csv_bam_set_frame)
    const void* owner = nullptr;
    bool chunk_ok = false;
    i64 n = 0, slim_bytes = 0, host_bytes = 0;
    std::vector<int64_t> rec_off, host_off;
    std::vector<uint32_t> rec_len;
    std::vector<int32_t> l_name, l_seq;
    i64 right = 0, fallback = 0, bytes_down = 0, bytes_up = 0;
    double ms_kernels = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&win[0], &win[1], &tab, &starts, &rows, &pack, &slim, &host, &cols}); }
};

// The index build (stage_index.hip.h), all stand-alone and grow-only.  blocks (the whole-file block table), refs
// (reference lengths and the offsets of their linear arrays), lin (the linear arrays) and counts live from csv_index_begin to
// csv_index_end: one build.  work (per record the two virtual offsets, bin and head flag; the scan's tables; the verdict; the runs) is
// dead when a csv_index_window returns; runs_h is its host copy of the runs.  The entries READ FrameState's rows and current window,
// which csv_frame_run left for them, and write nothing outside this struct; of the context they touch the stream and its first two
// timing events, nothing else.
struct IndexBuildState {
    Buf blocks, refs, lin, counts, work;
    i64 n_blocks = 0, n_lin = 0;
    int n_ref = -1;                            // -1: no build is open
    IxFormat fmt = ix_bai();                   // the scheme of the open build
    std::vector<i64> lin_off_h;                // n_ref + 1: the host's copy, for the checks of csv_index_end_loff
    double ms_loff = 0;                        // k_index_loff of the last CSI build
    std::vector<IxRun> runs_h;
    double ms_kernels = 0;
    i64 bytes_down = 0, bytes_up = 0, windows = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&blocks, &refs, &lin, &counts, &work}); }
};

// The coordinate sort of a BAM file (stage_bam_sort.hip.h), all stand-alone.  arena (the whole inflated stream at
// its own offsets, 32 bytes of slack behind it), hdr (the rewritten header), starts, key, len, perm[2], hist, tot, dst, tiles and
// verdict live from csv_sort_begin to csv_sort_end: one sort; csv_sort_end gives the arena back, the rest is grow-only.  slice: the
// gathered bytes of one csv_sort_slice, which DeflateState's buffers then compress where they lie.  csv_sort_append READS FrameState's
// current window when the reader frames on the device; nothing else of the context is touched but its stream and its first two
// timing events.
struct BamSortState {
    Buf arena, hdr, starts, key, len, perm[2], hist, tot, dst, tiles, verdict, slice;
    i64 arena_bytes = -1, hdr_bytes = 0, slice_bytes = 0, n = -1, total = 0;      // arena_bytes -1: no sort is open; n -1: not ordered yet
    const int* order = nullptr;                // the final permutation (NULL: the identity)
    std::vector<i64> off_h;
    std::vector<int32_t> len_h;
    double ms[4] = {0, 0, 0, 0};               // keys, sort (passes and dst), gather, deflate
    i64 bytes_up = 0, bytes_down = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&arena, &hdr, &starts, &key, &len, &perm[0], &perm[1], &hist, &tot, &dst, &tiles, &verdict, &slice}); }
};

// SAM text -> BAM (stage_sam.hip.h).  Everything lives for one csv_sam_to_bam call and is grow-only between calls:
// text - the window; nl / tab - its marks; rows / len / dst - the plan and its scan; stream - the window's part of the BAM stream, which
// DeflateState's buffers compress where it lies; carry - the bytes of a partial last block on their way in front of the next window's
// stream.  Nothing else of the context is touched but its stream, its staging block and its first three timing events.
struct SamState {
    Buf text, cnt, small, nl, tab, rows, len, dst, tiles, items, patches, stream, carry, names, names_tab, item_tab, item_bytes, patch_bits;
    i64 carry_bytes = 0;
    SamStats st;
    std::vector<int> cnt_h, item_line;
    std::vector<i64> nl_h, item_off, item_size;
    std::vector<uint8_t> item_rec;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&text, &cnt, &small, &nl, &tab, &rows, &len, &dst, &tiles, &items, &patches, &stream, &carry, &names, &names_tab, &item_tab, &item_bytes, &patch_bits}); }
};

// ---- The state of the engine (stage_upload / stage_run / stage_results.hip.h): the path csv_batch_upload -> csv_batch_run ->
// csv_batch_download / csv_batch_publish_* and the one-shot csv_cluster_batch.  One struct per concern, with the same kind of rule.

// CSV_* environment switches of the engine (timing / debugging aids), read by load_run_opts at the top of EVERY upload and
// nowhere else: csv_batch_run - a 36 us step - looks nothing up in the environment, and neither do the phases of an upload.
struct RunOpts {
    bool debug = false, debug_counters = false, debug_timing = false, no_fork = false, fork_always = false, no_swap = false, no_peek = false;
    bool no_pair_in_mid = false, no_publish = false;
    int  iw_grid = 0, gt_grid = 0, tier_fork_min = 1 << 30, mid_grid = 0, big_grid = 0;
    bool pub_inplace = false, no_reads_overlap = false;
    // the forms an upload may choose
    bool no_lazy = false, no_rows8 = false, no_delta16 = false, copy_stream = false, no_tiny = false;
    int  lazy_min = 64 << 10, delta16_min = 32 << 10, delta16_esc = 64, reads_gap = 1000000;
};

// The resident batch.  Every Buf is a slice of csv_ctx::arena that upload_impl plans and fills; the run's kernels read and write
// them through B (the DevBatch every kernel takes).  They live until the next upload - which re-plans the arena, after waiting
// for the device when the arena has to move - and nobody outside the engine reads them.  seg .. tile_info are slices of `tabs`
// (the small tables: one block, one copy).  h_seg / h_woff: the host copies of the segments and their prefix in w space, read
// by the downloads.  The flags are set by the upload and cleared by the next one, except: `ran` (set by a run, cleared by
// csv_batch_validate and by a rebuild, which also clears `uploaded`: it counts into the engine's counter block),
// copies_pending / unpack_pending / lazy_pending (a one-shot call's first run consumes them).
struct BatchState {
    Buf seg, woff, seg_drop, seg_gate, seg_err, tile_info, tabs;
    Buf a, b, rid, aux, a32, b32;
    Buf tile_lead;
    Buf ad16, anc;                             // CSV_IN_SIG_DELTA16: the gaps in w space; the anchor tables {per-tile offsets, w, value}
    Buf cluster_id, allele_id, partial, tile_cnt, item_rec, list_small, list_big, list_tiny, list_wide, ch_masks, tile_items;
    Buf item_cnt, item_base, item_chunk, sup_tmp;
    Buf t_rec, t_rec0;
    Buf sc_k, sc_x, sc_v1, sc_v2, sc_v3, sc_v4, sc_v5;
    Buf o_suprid;
    // the reads table as uploaded (r_*; its 16-bit forms rd16 .. rlesc) and its packed start-ordered form (s_* .. maxlen), the genotype scratch
    Buf reads_off, contig_len, r_start, r_end, r_primary, r_id;
    Buf rd16, ranc, rl16, rlesc;               // CSV_IN_READS_DELTA16: start gaps + their anchors, lengths + their escape rows / values
    Buf s_start, s_end, s_idp, cmax, cfirst, bfirst, span_len, maxlen, gt_over, gt_huge, gt_pool;
    std::vector<csv_segment> h_seg;
    std::vector<i64>         h_woff;
    DevBatch B;
    bool uploaded = false, ran = false, any_genotype = false, any_pair = false, any_tra_gt = false;
    bool delta16 = false;                      // the last upload rebuilt its position column from gaps (csv_batch_info 2)
    bool copies_pending = false;               // csv_cluster_batch: the column copies are still in flight behind ev_copy[0] / [1]
    bool unpack_pending = false; UnpackArgs unpack_args{}; int unpack_tiles = 0;      // k_unpack_a16 of the position column is still to be queued (one-shot calls: by the run)
    bool lazy_pending = false;                 // gate-first call: this upload's first run still has to fetch the gated rows from the caller's columns
    bool partial_cols = false;                 // ... and its device columns hold only the rows the kernels read (csv_batch_validate refuses)
    i64  lazy_bytes = 0;                       // bytes the bulk copy of this upload did NOT send (measurement aid: csv_batch_lazy_info)
    i64  n_sig_host = 0, n_reads = 0;
    int  upload_seq0 = 0;                      // run_seq when the resident batch was uploaded: later sequence numbers are runs of it
};

// The reads stage: the order of the uploaded reads table.  tcnt .. tblk are slices of csv_ctx::arena, planned by an upload
// whose table is not sorted (dead at the next upload); rstate (the stage's verdict on the table, on the device) and the gs_*
// buffers of the general sort (allocated on first use) stand alone and live as long as the context.  The flags belong to one
// upload and are reset by the next; reads_ready is also cleared when a run finds that the table needs the general sort.
// reuse_reads is the caller's (csv_batch_option) and survives uploads.
struct ReadsOrderState {
    Buf tcnt, ent, table, tblk;
    std::vector<int> h_tblk;                   // per tile of the reads table: the first chromosome block that begins at or after it (the source of an asynchronous copy)
    Buf rstate;
    Buf gs_chrom, gs_perm0, gs_perm1, gs_hist, gs_tot;          // general reads sort (fallback), allocated on first use
    bool rstate_dirty = true;                  // the reads-order state may hold an earlier upload's verdict
    int  reads_delta = 0;                      // bit 0: the last upload's reads starts crossed as gaps, bit 1: its ends as lengths, bit 2: id | primary packed (csv_batch_info 3)
    bool reads_early = false;                  // the last upload decoded the reads table's start column on side[1] (upload_reads)
    bool reads_ready = false;                  // the packed start-ordered reads table of this upload exists (a completed reads stage)
    bool reuse_reads = true;                   // ... and resident re-runs keep it (csv_batch_option CSV_OPT_REUSE_READS_ORDER)
    bool have_tab = false;                     // this upload issued copies of the reads table frame (reads_off, contig_len, columns) on side[2]
    bool reads_general = false;                // this batch's reads table needs the general sort (found out by a first run)
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&rstate, &gs_chrom, &gs_perm0, &gs_perm1, &gs_hist, &gs_tot}); }
};

// Results and their delivery.  o_rec / o_supsig and o_rec2 / o_supsig2 are the two result arenas (slices of csv_ctx::arena, dead
// at the next upload): runs alternate between them (`parity` = the arena of the last run), so that the k_publish of run k reads
// arena k & 1 on the publish stream `pub` while run k + 1 fills the other one.  cnt (stand-alone, 1024 bytes): the counters of
// arena 0 / 1 at +0 / +256, csv_batch_validate's at +512, the rebuild's row count at +768; h_cnt: the counters of the last
// download or instrumented run.  pend / pend_order / n_pend: the publishes in flight, oldest first; an upload waits for them and
// forgets them.  settled: a run of this upload has been downloaded synchronously (reads mode final, capacities known).  h_pub:
// the page-locked landing zones of the asynchronous publishes, 2 x {counters 256 B, status words}; pub_stage: per arena the
// device image of a block delivery (when the caller's result arrays sit back to back in page-locked memory, k_publish writes
// them into this image and the copy engine moves each run of adjacent arrays in one piece).  Both grow only, while no publish
// is in flight, and go with the context.
struct ResultState {
    Buf o_rec, o_supsig, o_rec2, o_supsig2;
    Buf cnt;
    DevCounters h_cnt;
    int  parity = 0;
    struct Pend { csv_batch_out* out = nullptr; bool live = false; } pend[2];
    int  pend_order[2] = {0, 0}, n_pend = 0;
    bool settled = false;
    hipStream_t pub = nullptr;
    hipEvent_t  ev_run[2] = {}, ev_pub[2] = {};
    char*  h_pub = nullptr;
    size_t h_pub_cap = 0;
    void*  pub_stage[2] = {nullptr, nullptr};
    size_t pub_stage_cap[2] = {0, 0};
    void own(std::vector<Buf*>& v) { v.push_back(&cnt); }
};

// The libm tables of cal_CIPOS (sqrt_table): stand-alone, sqrt_n entries each, grown - after a device synchronisation - to the
// longest segment any upload has seen, never shrunk; every batch's kernels read them.
struct TableState {
    Buf sqrt_tab, rcp_tab, cipk_tab;
    i64 sqrt_n = 0;
    void own(std::vector<Buf*>& v) { v.insert(v.end(), {&sqrt_tab, &rcp_tab, &cipk_tab}); }
};

}  // namespace

struct csv_ctx {
    // ---- what every entry shares
    int         device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side[3] = {};         // side streams: [0] mid + workgroup tier, [1] DUP/INV/TRA wavefront tier, [2] reads order + prefix max
    hipStream_t copy[N_COPY_STREAMS] = {};    // host -> device column copies (one DMA engine each)
    hipEvent_t  ev_init = nullptr, ev_sel = nullptr, ev_aux[3] = {}, ev_copy[N_COPY_STREAMS] = {}, ev_reads = nullptr, ev_anc = nullptr, ev_rd[5] = {};
    std::string err;
    hipEvent_t  ev[CSV_N_STAGES + 2] = {};
    Arena       arena;                         // the batch arena: planned afresh by every upload (BatchState, ReadsOrderState, ResultState slice it)
    Arena       scratch;                       // per-call scratch of the rebuild, the CIGAR scan and the split analysis
    Buf         flush;                         // csv_cache_flush scratch (stand-alone)
    // page-locked host staging: small tables on the way in, counters + call records + support lists on the way out
    char*  h_pin = nullptr;
    size_t h_pin_cap = 0;
    RunOpts opt;
    // two page-locked 64-bit words the device writes {run sequence, count}: items above 64 signatures (k_chain_apply), calls that
    // overflowed the first genotype pass (k_genotype<8192>); read when a LATER run of the same upload is planned
    volatile int* h_flag = nullptr;
    int*          d_flag = nullptr;
    int           run_seq = 0;
    int           n_cu = 256;              // compute units of the device
    bool          lds_set = false;         // the dynamic-LDS limits of the run's kernels are set (once per context)
    // ---- the engine (stage_upload / stage_run / stage_results; their lifetime rules: at the structs)
    BatchState bt; ReadsOrderState ro; ResultState res; TableState tab;
    // ---- the extraction-side stages (their lifetime rules: at the structs)
    PoolState pool; NameState nm; BamState bm; SaState sa; SeqState seq; VcfStrState vs; AlnState al; ReadsTabState rt;
    RebuildState rb; CigarState cg; SplitState sp; InflateState inf; FrameState fr; IndexBuildState ixb; DeflateState dfl; RefState ref; VcfEmitState ve; BamSortState bs; SamState sam;
};

namespace {

int fail(csv_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_TRY(c, call)                                                                                   \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return fail((c), CSV_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_));   \
    } while (0)

// a helper's status passed on (the helpers below set the error text themselves)
#define TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

int reserve(csv_ctx* c, Buf& b, size_t bytes)            // stand-alone grow-only buffer
{
    if (bytes <= b.cap) return CSV_OK;
    if (b.p) { HIP_TRY(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return fail(c, CSV_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
    b.cap = want;
    return CSV_OK;
}

// room for `bytes` in the page-locked staging block (grow-only; the caller makes sure no copy still uses the old one)
int pin_reserve(csv_ctx* c, size_t bytes)
{
    if (bytes <= c->h_pin_cap) return CSV_OK;
    if (c->h_pin) { HIP_TRY(c, hipHostFree(c->h_pin)); c->h_pin = nullptr; c->h_pin_cap = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, CSV_E_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    c->h_pin = (char*)p; c->h_pin_cap = want;
    return CSV_OK;
}

// room for `bytes` in a stand-alone buffer whose first `keep` bytes must survive (grows by copying, by half)
int grow_keep(csv_ctx* c, Buf& b, size_t bytes, size_t keep)
{
    if (bytes <= b.cap) return CSV_OK;
    const size_t want = bytes + bytes / 2 + 4096;
    void* p = nullptr;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return fail(c, CSV_E_NOMEM, "hipMalloc(%zu) for the name pool failed: %s", want, hipGetErrorString(e));
    if (keep > 0 && b.p) HIP_TRY(c, hipMemcpy(p, b.p, keep, hipMemcpyDeviceToDevice));
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = p; b.cap = want;
    return CSV_OK;
}

int commit(csv_ctx* c, Arena& A, const Plan& P)
{
    if (P.total > A.cap) {
        if (A.base) { HIP_TRY(c, hipFree(A.base)); A.base = nullptr; A.cap = 0; }
        const size_t want = P.total + P.total / 8 + 4096;
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return fail(c, CSV_E_NOMEM, "hipMalloc(%zu) for the batch arena failed: %s", want, hipGetErrorString(e));
        A.base = (char*)p; A.cap = want;
    }
    for (const auto& it : P.items) it.first->p = A.base + it.second;
    return CSV_OK;
}

// commit, waiting for the device first when the arena has to move: nothing may still be running out of the old one
int commit_synced(csv_ctx* c, Arena& A, const Plan& P)
{
    if (P.total > A.cap) HIP_TRY(c, hipDeviceSynchronize());
    return commit(c, A, P);
}

template <class T> T* dp(const Buf& b) { return (T*)b.p; }
int div_up(i64 a, i64 b) { return (int)((a + b - 1) / b); }

// a result column on its way to the caller: the rows of the copy tables of the stage entries
struct HostCol { void* host; const Buf* dev; i64 bytes; };

// host -> device on the context's stream; nothing to do for zero bytes
int h2d(csv_ctx* c, const Buf& b, const void* src, i64 bytes)
{
    if (bytes > 0) HIP_TRY(c, hipMemcpyAsync(b.p, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    return CSV_OK;
}

// device -> host on the context's stream.  A NULL `dst` is an output the caller did not ask for when `required` is false; when it is true the
// copy goes to HIP as it is, which reports the NULL.  Zero bytes are skipped either way (the HIP runtime's copy returns hipSuccess for no bytes before it checks a pointer).
int d2h(csv_ctx* c, void* dst, const Buf& b, i64 bytes, bool required)
{
    if (bytes > 0 && (dst || required)) HIP_TRY(c, hipMemcpyAsync(dst, b.p, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    return CSV_OK;
}

// len[i] bytes at dev_src + src_off[i] -> dst + dst_off[i] for i < n, on the device (k_frame_gather): src_off / len are the caller's
// host columns (checked by the caller, alive until it synchronises), dst_off lies in device memory; FrameState::cols carries the tables
int frame_gather(csv_ctx* c, i64 n, const uint8_t* dev_src, const int64_t* src_off, const int32_t* len, uint8_t* dst, const i64* dst_off)
{
    if (n <= 0) return CSV_OK;
    TRY(reserve(c, c->fr.cols, (size_t)n * 12 + 16));
    char* t = (char*)c->fr.cols.p;
    HIP_TRY(c, hipMemcpyAsync(t, src_off, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(t + (size_t)n * 8, len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    c->fr.bytes_up += n * 12;
    hipLaunchKernelGGL(k_frame_gather, dim3(std::min(div_up(n, 4), 8192)), dim3(256), 0, c->stream, dev_src, (const i64*)t, (const int*)(t + (size_t)n * 8), n, dst, dst_off);
    HIP_TRY(c, hipGetLastError());
    return CSV_OK;
}

// The device time of an entry in two phases around a host decision (count kernels, totals back and capacity check, emit
// kernels): events c->ev[0..3] on the context's stream; every *_end also collects launch errors.
struct TwoPhaseTimer {
    csv_ctx* c;
    bool emitted = false;
    int count_begin() { HIP_TRY(c, hipEventRecord(c->ev[0], c->stream)); return CSV_OK; }
    int count_end() { HIP_TRY(c, hipEventRecord(c->ev[1], c->stream)); HIP_TRY(c, hipGetLastError()); return CSV_OK; }
    int emit_begin() { HIP_TRY(c, hipEventRecord(c->ev[2], c->stream)); emitted = true; return CSV_OK; }
    int emit_end() { HIP_TRY(c, hipEventRecord(c->ev[3], c->stream)); HIP_TRY(c, hipGetLastError()); return CSV_OK; }
    int elapsed(float* ms)            // ms1 + ms2 once the stream is idle; ms1 alone while (or when) no emit phase ran
    {
        float ms1 = 0, ms2 = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms1, c->ev[0], c->ev[1]));
        if (emitted) HIP_TRY(c, hipEventElapsedTime(&ms2, c->ev[2], c->ev[3]));
        *ms = emitted ? ms1 + ms2 : ms1;
        return CSV_OK;
    }
};

// One key column of the LSD permutation sort (sort.hip.h): a pass per byte k < n_bytes whose bit is set in `mask`, over the bits first_shift + [8 k, 8 k + 8)
struct SortField { const void* col; int elem64; int first_shift; int n_bytes; unsigned mask; };

// The radix passes over `fields`, least significant field first: histogram, row sums, row scan, scatter; the permutation
// goes back and forth between perm0 and perm1.  Returns the final permutation (nullptr: no pass ran, the order is the rows').
const int* sort_passes(hipStream_t st, const SortField* fields, int n_fields, i64 n, int nunits, int* perm0, int* perm1, int* hist, int* tot, int* npass)
{
    const int nblk = div_up(nunits, 4);
    const int* pin = nullptr;
    int* pout = perm0;
    for (int f = 0; f < n_fields; f++)
        for (int byte = 0; byte < fields[f].n_bytes; byte++) {
            if (!((fields[f].mask >> byte) & 1u)) continue;
            SortPass SP{fields[f].col, fields[f].elem64, fields[f].first_shift + byte * 8, n, nunits, pin, pout, hist};
            hipLaunchKernelGGL(k_sort_hist, dim3(nblk), dim3(256), 0, st, SP);
            hipLaunchKernelGGL(k_sort_rowsum, dim3(256), dim3(256), 0, st, hist, nunits, tot);
            hipLaunchKernelGGL(k_sort_rowscan, dim3(256), dim3(256), 0, st, hist, nunits, tot);
            hipLaunchKernelGGL(k_sort_scatter, dim3(nblk), dim3(256), 0, st, SP);
            pin = pout;
            pout = (pout == perm0) ? perm1 : perm0;
            if (npass) ++*npass;
        }
    return pin;
}

}  // namespace
