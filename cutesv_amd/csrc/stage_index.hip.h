// stage_index.hip.h — the index build on the device (IndexBuildState in ctx.hip.h; index_core.h; k_index_rows / k_index_runs at the
// end of bam.hip.h): the reader's internal entries (csv_index_*, declared in index_core.h, called by bam_host.cpp
// alone).  The rows of a framed window stay in device memory (csv_frame_run with rows == NULL); what comes down per window is the
// verdict and one 32-byte row per run, and once at the end the linear arrays and the counts.  Host code; included by cutesv_hip.hip
// behind stage_frame.hip.h.

// a build begins: the block table and the reference lengths go up, the linear arrays become IX_NONE, the counts zero
int csv_index_begin(csv_ctx* c, int32_t n_ref, const ix_i64* l_ref, int64_t n_blocks, const ix_i64* uoff, const ix_i64* coff, const uint32_t* isize)
{
    const IxFormat bai = ix_bai();
    return csv_index_begin_fmt(c, &bai, n_ref, l_ref, n_blocks, uoff, coff, isize);
}

// ... under the binning scheme *fmt (index_core.h): a CSI build, or csv_index_begin's BAI
int csv_index_begin_fmt(csv_ctx* c, const IxFormat* fmt, int32_t n_ref, const ix_i64* l_ref, int64_t n_blocks, const ix_i64* uoff, const ix_i64* coff, const uint32_t* isize)
{
    if (!c) return CSV_E_INVALID;
    IndexBuildState& x = c->ixb;
    x.n_ref = -1;
    if (!fmt || !ix_format_ok(*fmt) || fmt->max_pos != ix_format(fmt->min_shift, fmt->depth).max_pos) return fail(c, CSV_E_INVALID, "bad index build: the binning scheme");
    if (n_ref < 0 || n_blocks < 1 || (n_ref > 0 && !l_ref) || !uoff || !coff || !isize) return fail(c, CSV_E_INVALID, "bad index build");
    for (i64 k = 0; k < n_blocks; k++)                                        // the kernels trust the table: contiguous, ascending
        if (isize[k] > 65536u || uoff[k] != (k ? uoff[k - 1] + (i64)isize[k - 1] : 0) || coff[k] < 0 || (k && coff[k] <= coff[k - 1]))
            return fail(c, CSV_E_INVALID, "bad index build: block %lld of the table", (long long)k);
    std::vector<i64> refs(2 * (size_t)n_ref + 1, 0);                          // l_ref, then lin_off (n_ref + 1)
    i64* lin_off = refs.data() + n_ref;
    for (int32_t r = 0; r < n_ref; r++) { refs[(size_t)r] = l_ref[r]; lin_off[r + 1] = lin_off[r] + ix_lin_entries(l_ref[r], *fmt); }
    const i64 n_lin = lin_off[n_ref], n_counts = 2 * (i64)n_ref + 1;
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(reserve(c, x.blocks, (size_t)n_blocks * 20 + 16));
    TRY(reserve(c, x.refs, refs.size() * 8));
    TRY(reserve(c, x.lin, (size_t)n_lin * 8 + 8));
    TRY(reserve(c, x.counts, (size_t)n_counts * 8));
    hipStream_t st = c->stream;
    char* t = (char*)x.blocks.p;
    HIP_TRY(c, hipMemcpyAsync(t, uoff, (size_t)n_blocks * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(t + (size_t)n_blocks * 8, coff, (size_t)n_blocks * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(t + (size_t)n_blocks * 16, isize, (size_t)n_blocks * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(x.refs.p, refs.data(), refs.size() * 8, hipMemcpyHostToDevice, st));
    if (n_lin > 0) HIP_TRY(c, hipMemsetAsync(x.lin.p, 0xff, (size_t)n_lin * 8, st));
    HIP_TRY(c, hipMemsetAsync(x.counts.p, 0, (size_t)n_counts * 8, st));
    HIP_TRY(c, hipStreamSynchronize(st));                                     // (the sources are the caller's and this function's)
    x.n_blocks = n_blocks; x.n_lin = n_lin; x.n_ref = n_ref; x.fmt = *fmt;
    x.lin_off_h.assign(lin_off, lin_off + n_ref + 1);
    x.ms_loff = 0;
    x.ms_kernels = 0; x.bytes_down = 0; x.windows = 0;
    x.bytes_up = n_blocks * 20 + (i64)refs.size() * 8;
    return CSV_OK;
}

// the n_records rows csv_frame_run left on the device, of the window whose first byte is stream byte win_u0; ordinal0: the ordinal of
// the first of them in the file; *carry: the record in front of it.  -> *verdict, and *runs = verdict->n_runs rows (host memory of the
// state, valid until the next call)
int csv_index_window(csv_ctx* c, int64_t n_records, int64_t win_u0, int64_t ordinal0, const IxCarry* carry, IxVerdict* verdict, const IxRun** runs)
{
    if (!c || !carry || !verdict || !runs) return CSV_E_INVALID;
    IndexBuildState& x = c->ixb;
    const FrameState& f = c->fr;
    *runs = nullptr;
    if (x.n_ref < 0) return fail(c, CSV_E_STATE, "no index build is open on this context");
    if (n_records < 1 || n_records != f.n_rows || (size_t)n_records * sizeof(FrRow) > f.rows.cap || win_u0 < 0 || ordinal0 < 0)
        return fail(c, CSV_E_INVALID, "bad index window: %lld records, the framed window has %lld", (long long)n_records, (long long)f.n_rows);
    const size_t n = (size_t)n_records;
    const size_t o_scan = 32 * n, o_tile = o_scan + 16 * n, o_tot = o_tile + scan_tile_bytes(n_records), o_ver = o_tot + 32, o_runs = o_ver + sizeof(IxVerdict), total = o_runs + 32 * n;
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(reserve(c, x.work, total));
    hipStream_t st = c->stream;
    char* t = (char*)x.work.p;
    const char* bt = (const char*)x.blocks.p;
    IndexArgs A{};
    A.win = dp<uint8_t>(f.win[f.cur]); A.win_n = f.win_n; A.win_u0 = win_u0;
    A.rows = dp<FrRow>(f.rows); A.n = n_records; A.ordinal0 = ordinal0; A.carry = *carry;
    A.blocks = IxBlocks{(const i64*)bt, (const i64*)(bt + (size_t)x.n_blocks * 8), (const uint32_t*)(bt + (size_t)x.n_blocks * 16), x.n_blocks};
    A.n_ref = x.n_ref; A.l_ref = dp<i64>(x.refs); A.lin_off = dp<i64>(x.refs) + x.n_ref;
    A.fmt = x.fmt;
    A.lin = dp<u64>(x.lin); A.counts = dp<u64>(x.counts);
    A.aux = (IxAux*)t; A.scan = (int4*)(t + o_scan); A.totals = (const i64*)(t + o_tot);
    A.verdict = (IxVerdict*)(t + o_ver); A.runs = (IxRun*)(t + o_runs);
    const int grid = div_up(n_records, 256);
    HIP_TRY(c, hipMemsetAsync(A.verdict, 0xff, sizeof(IxVerdict), st));       // bad = IX_NONE; k_index_runs writes the rest
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_index_rows, dim3(grid), dim3(256), 0, st, A);
    scan_counts(st, ScanArgs{n_records, A.scan, (i64*)(t + o_tile), (i64*)(t + o_tot)});
    hipLaunchKernelGGL(k_index_runs, dim3(grid), dim3(256), 0, st, A);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    HIP_TRY(c, hipGetLastError());
    IxVerdict V;
    HIP_TRY(c, hipMemcpyAsync(&V, A.verdict, sizeof V, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    x.ms_kernels += ms; x.windows++;
    x.bytes_down += (i64)sizeof V;
    if (V.n_runs < 0 || V.n_runs > n_records) return fail(c, CSV_E_INVALID, "index: inconsistent counts (%lld runs of %lld records)", (long long)V.n_runs, (long long)n_records);
    x.runs_h.resize((size_t)V.n_runs);
    if (V.n_runs > 0 && V.bad == IX_NONE) {                                  // (a refused window's runs are nobody's business)
        HIP_TRY(c, hipMemcpyAsync(x.runs_h.data(), A.runs, (size_t)V.n_runs * sizeof(IxRun), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        x.bytes_down += V.n_runs * (i64)sizeof(IxRun);
    }
    *verdict = V; *runs = x.runs_h.data();
    return CSV_OK;
}

// the build ends: the linear arrays (n_lin entries, as csv_index_begin laid them out) and the counts (2 * n_ref + 1) come down
int csv_index_end(csv_ctx* c, ix_u64* lin, int64_t n_lin, ix_u64* counts, int64_t n_counts)
{
    if (!c) return CSV_E_INVALID;
    IndexBuildState& x = c->ixb;
    if (x.n_ref < 0) return fail(c, CSV_E_STATE, "no index build is open on this context");
    if (n_lin != x.n_lin || n_counts != 2 * (i64)x.n_ref + 1 || (n_lin > 0 && !lin) || !counts) return fail(c, CSV_E_INVALID, "bad index build: the arrays' sizes");
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_lin > 0) HIP_TRY(c, hipMemcpyAsync(lin, x.lin.p, (size_t)n_lin * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts, x.counts.p, (size_t)n_counts * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    x.bytes_down += (n_lin + n_counts) * 8;
    x.n_ref = -1;
    return CSV_OK;
}

// a CSI build ends: pairs = n_pairs {ref, bin} of bins that hold records -> loff[k], the first touched linear entry from the bin's first
// window on (IX_NONE: none), by k_index_loff; the counts come down, the linear arrays do not.  Everything the kernel indexes with is
// checked here: the pair count against the regular bins of all references, ref, bin < ix_n_bins, the first window inside the
// reference's entries
int csv_index_end_loff(csv_ctx* c, int64_t n_pairs, const uint32_t* pairs, ix_u64* loff, ix_u64* counts, int64_t n_counts)
{
    if (!c) return CSV_E_INVALID;
    IndexBuildState& x = c->ixb;
    if (x.n_ref < 0) return fail(c, CSV_E_STATE, "no index build is open on this context");
    const i64 n_bins = (i64)ix_n_bins(x.fmt);
    if (n_counts != 2 * (i64)x.n_ref + 1 || !counts || n_pairs < 0 || n_pairs > n_bins * (i64)x.n_ref || (n_pairs > 0 && (!pairs || !loff)))
        return fail(c, CSV_E_INVALID, "bad index build: %lld bins of %d references", (long long)n_pairs, x.n_ref);
    std::vector<i64> span(2 * (size_t)n_pairs);                               // at, then end: entries of the whole linear array
    for (i64 k = 0; k < n_pairs; k++) {
        const uint32_t ref = pairs[2 * k], bin = pairs[2 * k + 1];
        if (ref >= (uint32_t)x.n_ref || (i64)bin >= n_bins) return fail(c, CSV_E_INVALID, "bad index build: bin %u of reference %u", bin, ref);
        const i64 bot = ix_bin_bot(bin, x.fmt), entries = x.lin_off_h[ref + 1] - x.lin_off_h[ref];
        if (bot < 0 || bot >= entries) return fail(c, CSV_E_INVALID, "bad index build: bin %u begins behind the windows of reference %u", bin, ref);
        span[(size_t)k] = x.lin_off_h[ref] + bot; span[(size_t)(n_pairs + k)] = x.lin_off_h[ref + 1];
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (n_pairs > 0) {
        TRY(reserve(c, x.work, (size_t)n_pairs * 24));
        char* t = (char*)x.work.p;
        HIP_TRY(c, hipMemcpyAsync(t, span.data(), (size_t)n_pairs * 16, hipMemcpyHostToDevice, st));
        IndexLoffArgs A{dp<u64>(x.lin), (const i64*)t, (const i64*)(t + (size_t)n_pairs * 8), (u64*)(t + (size_t)n_pairs * 16), n_pairs};
        HIP_TRY(c, hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(k_index_loff, dim3((unsigned)std::min<i64>(div_up(n_pairs, 4), 4096)), dim3(256), 0, st, A);
        HIP_TRY(c, hipEventRecord(c->ev[1], st));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(loff, A.loff, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipMemcpyAsync(counts, x.counts.p, (size_t)n_counts * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (n_pairs > 0) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        x.ms_kernels += ms; x.ms_loff = ms;
    }
    x.bytes_up += n_pairs * 16;
    x.bytes_down += (n_pairs + n_counts) * 8;
    x.n_ref = -1;
    return CSV_OK;
}

double csv_index_loff_ms(csv_ctx* c) { return c ? c->ixb.ms_loff : 0; }

int csv_index_counters(csv_ctx* c, double* ms_kernels, int64_t* bytes_down, int64_t* bytes_up, int64_t* windows)
{
    if (!c) return CSV_E_INVALID;
    const IndexBuildState& x = c->ixb;
    if (ms_kernels) *ms_kernels = x.ms_kernels;
    if (bytes_down) *bytes_down = x.bytes_down;
    if (bytes_up) *bytes_up = x.bytes_up;
    if (windows) *windows = x.windows;
    return CSV_OK;
}
