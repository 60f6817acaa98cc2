/*
 * cutesv_hip.h — C ABI of libcutesv_hip.so, the MI355X (gfx950) implementation of
 * cuteSV's signature clustering-and-refinement stage and its genotyping re-cluster.
 *
 * Every entry point replaces one piece of the reference's Python interface for this
 * path.  Reference citations are into /root/reference/src/cuteSV/ (v2.1.4):
 *   INDEL = cuteSV_resolveINDEL.py   DUP = cuteSV_resolveDUP.py   INV = cuteSV_resolveINV.py
 *   TRA   = cuteSV_resolveTRA.py     GT  = cuteSV_genotype.py     MAIN = cuteSV (main script)
 *
 * Boundary rules:
 *   - plain pointers and sizes only; the caller owns every host buffer, the library
 *     never retains a host pointer after a call returns;
 *   - device memory belongs to a per-process context (grow-only arena, one HIP stream);
 *   - a context is not thread-safe; distinct contexts are independent; create it
 *     AFTER fork (one HIP device per worker process, as MAIN:1113 uses one task per
 *     pool worker);
 *   - errors are returned as non-zero ints, never abort(); text via csv_last_error().
 *
 * The same structs are consumed by oracle/liboracle.so (csvo_cluster_batch), the CPU
 * restatement used only by tests/, smoke() and bench.py's cpu_baseline leg.
 */
#ifndef CUTESV_HIP_H
#define CUTESV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSV_ABI_VERSION 9

/* SV types: one (chromosome, type) pair is one segment == one reference pool task
 * (MAIN:1116-1189).  Order of the enum is irrelevant to results. */
enum { CSV_DEL = 0, CSV_INS = 1, CSV_DUP = 2, CSV_INV = 3, CSV_TRA = 4 };

enum {
    CSV_OK = 0,
    CSV_E_INVALID = 1,   /* bad argument / unsupported combination (e.g. TRA + genotype without contig_len) */
    CSV_E_CAPACITY = 2,  /* output arrays too small; n_calls / n_support hold the need */
    CSV_E_HIP = 3,       /* a HIP runtime call failed; see csv_last_error */
    CSV_E_NOMEM = 4,
    CSV_E_UNSORTED = 5,  /* csv_batch_validate: a segment is not in the rebuild order; or CSV_IN_READS_SORTED was promised
                            and a reads block is not sorted by start */
    CSV_E_STATE = 6      /* run/download without a preceding upload */
};

/*
 * One (chromosome, SV type) task.  The scalar fields are the positional arguments of the
 * reference's run_* tuples:
 *   DEL/INS  INDEL:17-18, 222-223  (read_count, threshold_gloab, max_cluster_bias,
 *            minimum_support_reads, action, remain_reads_ratio)
 *   DUP      DUP:17-18   (read_count, max_cluster_bias, sv_size, action, MaxSize)
 *   INV      INV:6-7     (read_count, max_cluster_bias, sv_size, action, MaxSize)
 *   TRA      TRA:30      (read_count, overlap_size, max_cluster_bias, action, gt_round)
 */
typedef struct csv_segment {
    int32_t svtype;             /* CSV_DEL..CSV_TRA */
    int32_t chrom;              /* index into reads_off[] (selects the reads block) */
    int64_t sig_begin;          /* [sig_begin, sig_end) in the signature columns */
    int64_t sig_end;
    int64_t max_cluster_bias;   /* INDEL:61, DUP:35, INV:56, TRA:65 */
    double  diff_ratio;         /* INDEL threshold_gloab (INDEL:138) / TRA overlap_size (TRA:134,211) */
    double  remain_reads_ratio; /* INDEL:46-47,169 (clamped to <= 1 by the library as well) */
    int64_t sv_size;            /* DUP:112 / INV:132 minimum size */
    int64_t max_size;           /* DUP:112 / INV:134 MaxSize, -1 = unlimited */
    int64_t gt_bias;            /* genotype half window: DEL max_cluster_bias (INDEL:103),
                                   INS 1000 (INDEL:312), DUP/INV max_cluster_bias (DUP:72, INV:94),
                                   TRA max_cluster_bias (TRA:164-166) */
    int32_t read_count;         /* min_support */
    int32_t min_support_reads;  /* min(min_support, 5), MAIN:1124 */
    int32_t genotype;           /* the reference's `action` flag */
    int32_t gt_round;           /* TRA only: --gt_round, the iteration cap of count_coverage (GT:62-93) */
} csv_segment;

/*
 * Flat signature / reads columns.  Within a segment the rows are in
 * the reference's sorted, adjacent-deduplicated order (MAIN:764-802, 958-969).
 *   a        int(pos) (DEL/INS)  | pos1 (DUP/INV/TRA)
 *   b        length (DEL/INS)    | pos2 (DUP/INV/TRA)
 *   read_id  interned read name; equal ids <=> equal names
 *   aux      INS: len(inserted sequence) | INV: strand code | TRA: chr2_rank*8 + BND type code (A..D = 0..3,
 *            codes 4..7 = any other BND type:
 *            the library emits nothing for it, TRA:154-155) | DEL/DUP: ignored
 * Reads table (MAIN:733): one block per chromosome (reads_off), rows in ANY order inside a block — the reference's
 * block is the concatenation of per-worker extraction batches, stably sorted by chromosome only (MAIN:810), and
 * overlap_cover sorts its sweep events itself (GT:101-109).  csv_batch_run brings every block into stable start order
 * on the device (stage "reads_order": whole sorted runs are moved when the block is a permutation of disjoint sorted
 * runs, which is what MAIN:697-735 produces; a general stable radix sort otherwise).  CSV_IN_READS_SORTED skips that.
 */
enum {
    CSV_IN_PER_SIG = 1,       /* also produce the per-signature outputs cluster_id / allele_id (csv_batch_download may
                                 then be given those arrays); without it the kernels skip 8 B of stores per signature */
    CSV_IN_READS_SORTED = 2,  /* caller's promise: every reads block is already sorted by r_start (checked on the
                                 device: CSV_E_UNSORTED if not) */
    CSV_IN_SIG_I32 = 4,       /* a and b point to int32_t columns (positions and lengths of a genome fit 31 bits; a third
                                 less data on the link: 67 -> 45 MB for a 30x genome); widened on the device */
    CSV_IN_READS_I32 = 8,     /* r_start and r_end point to int32_t columns */
    CSV_IN_DEVICE_COLUMNS = 16, /* a, b, read_id and aux are DEVICE pointers (memory of this context's GPU, e.g. csv_rebuild_out.dev_* of
                                 a csv_rebuild_signatures call with CSV_RB_KEEP_ON_DEVICE): the columns move device to device
                                 (HBM rate) instead of crossing PCIe twice; the reference's dataflow rebuild -> cluster
                                 (MAIN:750-857 -> 1113-1199) without a host round trip */
    CSV_IN_READS_DELTA16 = 64, /* (ABI v8, with CSV_IN_READS_I32) r_delta / r_len16 (either or both) are given: the reads table's start column
                                 crosses the link as 16-bit gaps (a block is a concatenation of start-sorted runs, MAIN:697-735, 810: a 30x
                                 genome's neighbours are ~0.5 kb apart) and its end column as 16-bit lengths (HiFi reads are < 64 kb), both
                                 rebuilt on the device: 13 -> 9 bytes per read, the bulk of a genotyping call's upload */
    CSV_IN_READS_DEVICE = 128, /* (with CSV_IN_READS_I32) r_start, r_end, r_primary and r_id are DEVICE pointers (memory of this context's GPU,
                                 e.g. what csv_reads_batch_columns hands out): the four columns move device to device at upload, so the
                                 caller may change its memory once the upload (or the one-shot call) has returned.  reads_off and
                                 contig_len stay host arrays.  CSV_E_INVALID without CSV_IN_READS_I32, or together with
                                 CSV_IN_READS_DELTA16, r_delta, r_len16 or r_idp: those forms read r_start on the host */
    CSV_IN_SIG_DELTA16 = 32   /* (ABI v8, with CSV_IN_SIG_I32, host columns) a_delta / a_esc_* are given: the position column crosses
                                 the link as 16-bit gaps - the rebuild order (MAIN:764-802) makes it non-decreasing inside a segment,
                                 a 30x genome's neighbours are ~1 kb apart - and is rebuilt on the device (k_unpack_a16): 11.1 -> 5.6 MB
                                 for a 30x genome, the largest single transfer of a gate-first call.  `a` must still be given (the
                                 library reads a few rows of it on the host; every other path uses it as before) */
};
typedef struct csv_batch_in {
    int32_t            n_seg;
    int32_t            n_chrom;
    const csv_segment* seg;
    int64_t            n_sig;
    const int64_t*     a;
    const int64_t*     b;
    const int32_t*     read_id;
    const int32_t*     aux;
    const int64_t*     reads_off;   /* n_chrom + 1 offsets; NULL when no segment genotypes */
    int64_t            n_reads;
    const int64_t*     r_start;
    const int64_t*     r_end;
    const uint8_t*     r_primary;
    const int32_t*     r_id;
    const int64_t*     contig_len;  /* n_chrom reference lengths (bamfile.get_reference_length, TRA:264,291); NULL unless a
                                       TRA segment genotypes */
    int32_t            flags;       /* CSV_IN_* */
    int32_t            reserved;
    /* (ABI v8) CSV_IN_SIG_DELTA16: a_delta[i] = a[i] - a[i - 1] where that lies in [0, 0xFFFF) and i > 0, else 0xFFFF and row i is listed
     * in a_esc_row (ascending) with a_esc_val = a[i].  n_sig entries; built once per store (SigStore.pinned()).  Rows that begin a
     * segment or a chain tile need no escape: the library anchors them itself.  NULL / 0 without the flag. */
    const uint16_t*    a_delta;
    int64_t            n_esc;
    const int64_t*     a_esc_row;
    const int32_t*     a_esc_val;
    /* (ABI v8, optional, with CSV_IN_SIG_I32) the length and read-id columns once more, interleaved: rows8[2 * i] = b[i],
     * rows8[2 * i + 1] = read_id[i], in page-locked memory.  A gate-first csv_cluster_batch (csv_batch_info 0) then reads the rows of
     * the clusters that pass the size gate (INDEL:62-64, 86) out of THIS array: a run of ~20 rows is 3-4 PCIe lines of 64 bytes
     * instead of 2-3 in each of two columns (the fetch is the largest item of such a call).  b and read_id must still be given. */
    const int32_t*     rows8;
    /* (ABI v8) CSV_IN_READS_DELTA16.  r_delta[i] = r_start[i] - r_start[i - 1] where that lies in [0, 0xFFFF) and i > 0, else 0xFFFF and
     * row i is listed in r_esc_row (ascending) with r_esc_val = r_start[i] (the first row of every sorted run is one).  r_len16[i] =
     * r_end[i] - r_start[i] where that lies in [0, 0xFFFF), else 0xFFFF and row i is listed in l_esc_row (ascending) with l_esc_val =
     * r_end[i].  n_reads entries each; r_start / r_end must still be given (the library reads a few rows of r_start on the host).
     * Either pointer may be NULL.  A column that is mostly escapes (shuffled blocks; ultra-long reads for r_len16) travels as itself. */
    const uint16_t*    r_delta;
    int64_t            n_r_esc;
    const int64_t*     r_esc_row;
    const int32_t*     r_esc_val;
    const uint16_t*    r_len16;
    int64_t            n_l_esc;
    const int64_t*     l_esc_row;
    const int32_t*     l_esc_val;
    /* (ABI v8, optional) r_idp[i] = r_id[i] | r_primary[i] << 31: the read id and the primary flag in one word (the form the device
     * keeps them in anyway).  When given, r_primary / r_id do not cross the link (5 -> 4 bytes per read); both must still be valid
     * pointers for the paths that read them on the host. */
    const uint32_t*    r_idp;
} csv_batch_in;

/*
 * Caller-allocated structure-of-arrays result.  One entry per candidate SV ("call"), in the
 * reference's emission order: segments in input order, clusters in file order, alleles /
 * sub-clusters in the order the reference appends them (INDEL:163-219, DUP:95-131, INV:124-203,
 * TRA:131-254).  Field meaning per type:
 *             bp1                  bp2                    support             search_pos
 *   DEL   int(breakpointStart)  int(signalLen) (>0)   allele read count    search_threshold (INDEL:177)
 *   INS   int(breakpointStart)  int(signalLen)        allele read count    = bp1 (INDEL:415)
 *   DUP   breakpoint_1          breakpoint_2          unique reads         -
 *   INV   breakpoint_1          breakpoint_2          unique reads         -
 *   TRA   int(sum p1 / n)       int(sum p2 / n)       unique reads         -
 * cipos / cilen: the integer inside cal_CIPOS's "-%d,%d" (GT:58-60), DEL/INS only.
 * seq_pick: INS only, global signature index whose sequence is sliced for ALT (INDEL:399-403).
 * call_aux: aux of the cluster's first signature (INV strand / TRA chr2,type).
 * dr / dv / gl_idx: genotype read counts (GT:161-173) and the index of cal_GL's result
 *   (GT:33-56) in the table defined by csv_gl_index(); -1 when the segment is not genotyped.
 *   TRA: call_gt / count_coverage (TRA:258-309, GT:62-93) evaluated over the READS TABLE
 *   instead of a BAM re-fetch: `fetch(chr, s, e)` = the reads of the chromosome's block with start < e and
 *   end > s, in block order; flag in [0, 16] = r_primary.  Identical to the reference whenever the BAM holds
 *   no alignment inside the two windows that the reads table drops (secondary flag 256/272, mapq < min_mapq,
 *   MAIN:711-733).  count_coverage's give-up status (-1) is dr = -1, gl_idx = -1 ("./.", DR ".").
 * support_off/support_sig: CSR list of the signatures whose read names form the call's
 *   read list, in reference order where that order is deterministic.
 * cluster_id / allele_id: optional per-signature outputs (NULL to skip; they need CSV_IN_PER_SIG on the batch,
 *   csv_cluster_batch sets it by itself when either array is given): dense id of the chained cluster a signature
 *   belongs to, and the index of the call (0-based, global) it supports or -1.
 * seg_status: optional (NULL to skip) n_seg words of CSV_SEG_* bits.  The reference has no size limits
 *   (INDEL:110-136, GT:95-159) and neither has this library; the only per-segment condition left is a length / pos2
 *   value outside [0, 2^42) (the clusters holding one emit nothing, every other cluster of the batch is unaffected;
 *   main_ctrl swallows a failing task the same way, MAIN:1193-1199).
 * (ABI v7) A caller that does not need a field does not pay for its trip across PCIe: call_cluster, call_aux, cipos, cilen,
 *   search_pos, seq_pick, dr, dv and gl_idx may each be NULL (not written); call_seg, bp1, bp2 and support are always required.
 *   `flags`: CSV_OUT_NO_SUPPORT_LIST - support_off / support_sig / support_sig32 are not written and may be NULL (`support` still
 *   holds every call's read count, n_support the total): read names reach the VCF only under --report_readid (GT:263-458), and
 *   the list is half of a discovery run's result bytes.  CSV_OUT_COORD_I32 - bp1, bp2, search_pos and seq_pick point to int32_t
 *   arrays (only with CSV_IN_SIG_I32 columns, whose coordinates fit by construction; CSV_E_INVALID otherwise).
 */
enum { CSV_SEG_KEY_RANGE = 1 };
enum { CSV_OUT_NO_SUPPORT_LIST = 1, CSV_OUT_COORD_I32 = 2 };
typedef struct csv_batch_out {
    int64_t  cap_calls;
    int64_t  cap_support;
    int64_t  n_calls;       /* out */
    int64_t  n_support;     /* out */
    int64_t  n_clusters;    /* out: chained clusters over the whole batch */
    int32_t* call_seg;
    int32_t* call_cluster;
    int32_t* call_aux;
    int64_t* bp1;
    int64_t* bp2;
    int32_t* support;
    int32_t* cipos;
    int32_t* cilen;
    int64_t* search_pos;
    int64_t* seq_pick;
    int32_t* dr;
    int32_t* dv;
    int32_t* gl_idx;
    int64_t* support_off;   /* cap_calls + 1 */
    int64_t* support_sig;   /* cap_support */
    int32_t* cluster_id;    /* n_sig or NULL */
    int32_t* allele_id;     /* n_sig or NULL */
    int32_t* seg_status;    /* n_seg or NULL */
    int32_t* support_sig32; /* (ABI v6) cap_support or NULL: the support list as int32 - a batch holds fewer than 2^31 signatures -
                               INSTEAD of support_sig (exactly one of the two is given): half the bytes of the largest result
                               array on the link */
    int32_t  flags;         /* (ABI v7) CSV_OUT_* */
    int32_t  reserved;
} csv_batch_out;

/* Per-kernel device timings of one csv_batch_run, measured with HIP events recorded on the
 * context's stream around every launch (only when stats != NULL; the plain run records nothing).
 * Kernel names: csv_stage_name(i); unused slots are 0. */
#define CSV_N_STAGES 24
typedef struct csv_run_stats {
    float   ms_total;
    float   ms_stage[CSV_N_STAGES];
    int64_t n_clusters;
    int64_t n_work_wave;    /* clusters refined by the one-wavefront-per-cluster tier */
    int64_t n_work_block;   /* clusters refined by the workgroup (LDS / global scratch) tier */
    int64_t n_calls;
    int64_t n_support;
} csv_run_stats;

typedef struct csv_ctx csv_ctx;

int         csv_abi_version(void);
/* sizeof() of the ABI's structs as this library was compiled (which: 0 csv_segment, 1 csv_batch_in, 2 csv_batch_out,
 * 3 csv_run_stats, 4 csv_rebuild_in, 5 csv_rebuild_out, 6 csv_vcf_in, 7 csv_rows_in, 8 csv_cigar_in, 9 csv_cigar_out, 10 csv_split_in,
 * 11 csv_split_out; -1 otherwise): lets a binding
 * check its own mirror of the layouts at load time. */
int         csv_struct_size(int which);
int         csv_device_count(int* n);
/* (ABI v7) PCI bus id of a device ("0000:c1:00.0") and its compute-unit count: what a multi-process launcher logs per rank to show
 * that N ranks sit on N distinct GPUs (the reference's pool workers have no placement: MAIN:1113).  Returns CSV_OK. */
int         csv_device_info(int device_id, char* pci_bus_id, int cap, int* n_cu);
int         csv_ctx_create(int device_id, csv_ctx** out);
void        csv_ctx_destroy(csv_ctx* ctx);
const char* csv_last_error(const csv_ctx* ctx);
const char* csv_stage_name(int stage);

/* One-shot: H2D, all kernels, D2H.  Replaces the bodies of resolution_DEL/INS/DUP/INV/TRA
 * (INDEL:17-108, 222-317; DUP:17-77; INV:6-99; TRA:30-104) and of call_gt -> overlap_cover
 * -> assign_gt (INDEL:441-479, DUP:137-181, INV:208-252, GT:95-173) for every segment of
 * the batch at once. */
int csv_cluster_batch(csv_ctx* ctx, const csv_batch_in* in, csv_batch_out* out);

/* Resident mode: the same work split at the PCIe boundary, so a caller (or bench.py) can
 * keep the columns in HBM and run the kernels repeatedly. */
int csv_batch_upload(csv_ctx* ctx, const csv_batch_in* in);
/* csv_batch_run only enqueues work (it returns before the kernels finish; csv_batch_download / csv_ctx_sync wait) and never
 * waits for the device.  A run of an upload that has been run before launches the refine tiers above 64 signatures only if
 * that earlier run reported clusters of that size (one page-locked word the device writes; same columns and parameters
 * give the same tiers); CSV_NO_PEEK=1 in the environment launches every tier always. */
int csv_batch_run(csv_ctx* ctx, csv_run_stats* stats /* nullable */);
int csv_batch_download(csv_ctx* ctx, csv_batch_out* out);
int csv_ctx_sync(csv_ctx* ctx);
/* (ABI v7) Pipelined delivery for a resident caller that runs batch after batch (or one batch again and again): the result of run
 * k is written into the caller's page-locked arrays by the device (as csv_batch_download does) on a stream of its own WHILE run
 * k + 1 computes - consecutive runs alternate between two result arenas on the device.  csv_batch_publish_async starts the
 * delivery of the LAST run's result into `out` and returns at once; csv_batch_publish_wait blocks until the OLDEST delivery in
 * flight is complete, fills n_calls / n_support / n_clusters / seg_status of its result struct - returned through `done` - and
 * returns its status (CSV_E_CAPACITY etc.).  At most two deliveries in flight, each into arrays of its own; every array must be
 * page-locked; no per-signature outputs; the upload must have been downloaded once synchronously before (that settles how its
 * reads table is ordered).  The sequence  run, async(A), run, async(B), wait -> A, run, async(A), wait -> B ...  keeps the link
 * busy under the kernels.  HOW the result crosses depends on where the caller put the arrays: arrays that sit exactly back to back
 * in page-locked memory (at most three such runs: e.g. every per-call array and the support list carved out of ONE csv_host_alloc
 * block, no gaps) are written as a device image behind the run's kernels and moved by the copy engine, one transfer per run of
 * arrays - in full, i.e. cap_calls / cap_support elements each: size them from the first download; scattered arrays are written in
 * place by a kernel on a stream of its own.  The first form is the one that overlaps: a kernel storing across PCIe holds up every
 * kernel boundary of the run beside it.  Elements beyond n_calls / n_support are unspecified in both forms.
 * No counterpart in the reference (its workers return pickled rows through a pipe, MAIN:1191-1197). */
int csv_batch_publish_async(csv_ctx* ctx, csv_batch_out* out);
int csv_batch_publish_wait(csv_ctx* ctx, csv_batch_out** done /* nullable */);
/* How the reads table of the last completed run was brought into start order: 0 = the caller promised sorted blocks,
 * 1 = whole sorted runs were moved (or nothing had to move), 2 = the general stable radix sort; -1 = no reads table. */
int csv_batch_reads_mode(const csv_ctx* ctx);
/* (ABI v7) What the last upload of this context did at the PCIe boundary: which = 0: 1 when csv_cluster_batch took the
 * gate-first form (page-locked b / read_id / aux columns: only the position column travels in bulk, the rows of the clusters
 * that pass the size gate - INDEL:62-64, 86 - are read out of the caller's columns by the device), else 0; which = 1: the
 * bytes of signature columns the bulk copy therefore did not send (ABI v8: including the half of the position column that
 * CSV_IN_SIG_DELTA16 saves); which = 2 (ABI v8): 1 when the position column crossed as 16-bit gaps; which = 3 (ABI v8): bit 0 / bit 1 when the reads table's
 * starts / ends crossed as 16-bit gaps / lengths.  A measurement aid
 * (bench.py's pcie object). */
int csv_batch_info(const csv_ctx* ctx, int which, int64_t* value);
/* Context options.  CSV_OPT_REUSE_READS_ORDER (default 1): the start-ordered, packed copy of the reads table that the first
 * csv_batch_run after an upload builds is kept for later runs of the SAME upload (a resident caller that re-runs a batch,
 * e.g. with other segment scalars, does not re-order millions of reads every time); 0 rebuilds it in every run.
 * csv_cluster_batch always builds it (every call is a new upload). */
enum { CSV_OPT_REUSE_READS_ORDER = 1 };
int csv_batch_option(csv_ctx* ctx, int option, int value);

/* Page-locked host memory.  Columns that live in it (or in a registered caller buffer) are copied asynchronously, so the
 * kernels start while the later columns are still on the link; a csv_cluster_batch call whose b / read_id / aux columns live in
 * it copies only the position column and lets the device read the rows it needs from the others (gate-first; batches of at
 * least CSV_LAZY_MIN = 65 536 signatures, CSV_NO_LAZY=1 in the environment switches it off); RESULT arrays that live in it are filled in place by the
 * device (csv_batch_download / csv_cluster_batch then cost one synchronisation: no staging copy, no host-side unpack) -
 * all of bp1 ... support_sig must be page-locked for that, seg_status and the per-signature arrays may be anywhere.
 * Memory from csv_host_alloc / csv_host_register must be released through csv_host_free / csv_host_unregister.  No
 * counterpart in the reference (its pool workers unpickle tuples, INDEL:52-58).  csv_host_alloc needs no context; the
 * memory is usable from every context of the process. */
int  csv_host_alloc(int64_t bytes, void** out);
void csv_host_free(void* p);
int  csv_host_register(void* p, int64_t bytes);
int  csv_host_unregister(void* p);

/* Optional check of the input order contract on the uploaded batch: inside every segment the rows must be
 * strictly increasing in the reference's rebuild sort key (cuteSV main script :764-802; adjacent duplicates
 * removed, :958-969).  Returns CSV_E_UNSORTED otherwise.  One pass over the columns; not part of csv_batch_run. */
int csv_batch_validate(csv_ctx* ctx);

/* Measurement aid (bench.py's roofline object): device-to-device copy bandwidth of this GPU, read + write bytes
 * over the best of `reps` hipMemcpyAsync calls of `bytes` bytes, in GB/s.  No counterpart in the reference. */
int csv_measure_copy_bandwidth(csv_ctx* ctx, int64_t bytes, int reps, double* gb_per_s);
/* Measurement aid: evict the GPU's caches (per-XCD L2s and the 256 MiB Infinity Cache) by overwriting a scratch buffer of
 * `bytes` bytes on the context's stream (allocated on first use), so that the next csv_batch_run finds its columns in
 * HBM only: the "cold" figures of bench.py.  No counterpart in the reference. */
int csv_cache_flush(csv_ctx* ctx, int64_t bytes);

/* cal_GL's domain after its special cases and rescale_read_counts (GT:25-37): returns the
 * table index the device writes into gl_idx for (DR, DV) = (c0, c1).  Host-side helper so
 * the Python shim and the tests share one definition with the kernels. */
int32_t csv_gl_index(int64_t c0, int64_t c1);
#define CSV_GL_TABLE_SIZE (101 * 101 + 2)

/* ---------------------------------------------------------------------------------------------
 * Rebuild step on the GPU: unsorted signature rows -> the order contract of
 * process_process_sigs_type (cuteSV main script :750-857): rows sorted by
 *   (segment, [aux for INV / TRA segments], a, b, read_id)           (:764-802 sort keys)
 * with adjacent exact duplicates removed (:958-969).  `seg_id` is the caller's ordinal of the row's
 * (SV type, chromosome) pair in the order the segments should come out; seg_aux_major[s] = 1 for INV and
 * TRA segments (strand / chr2,type sort before the position).  Stable LSD radix sort of a row permutation,
 * 8 bits per pass, zero bytes skipped; then gather + de-duplication.  Outputs are caller-allocated with
 * room for n rows; src_row[i] = input row of output row i (to carry payloads such as INS sequences).
 */
enum {
    CSV_RB_KEEP_ON_DEVICE = 1,       /* csv_rebuild_in.flags: the sorted columns stay in device memory (csv_rebuild_out.dev_*, valid
                                        until the context's next csv_rebuild_signatures / csv_cigar_signatures / csv_split_signatures
                                        call); host output arrays that are NULL are not written */
    CSV_RB_FROM_POOL = 2,            /* the rows are the context's device-resident signature pool (below): n, seg_id, a, b, read_id and
                                        aux of csv_rebuild_in are ignored; a row's read index is replaced by read_rank[index] (the
                                        rank of the read's NAME: string order is the caller's business, or the library's with
                                        CSV_RB_RANK_FROM_NAMES below); src_row numbers pool rows */
    CSV_RB_RANK_FROM_NAMES = 4,      /* with CSV_RB_FROM_POOL: read_rank / n_rank are ignored; a row's read index is replaced by the rank
                                        of that index in the context's NAME pool (csv_name_ranks below; computed first when an append
                                        made the cached ranks stale).  A row whose read index is >= the name count fails the call with
                                        CSV_E_INVALID, like every other row the sort cannot take; the context stays usable */
    CSV_RB_TIES_FROM_SEQS = 8        /* with CSV_RB_FROM_POOL and seg_nodedup, without tie_order (CSV_E_INVALID otherwise): the tie groups of
                                        the keep-every-row segments are settled on the device from the context's sequence pool
                                        (csv_seq_pool_* below) under exactly the contract of csv_tie_order_fn as extract's INS rows
                                        need it - inside a group rows order by sequence (unsigned bytes, a prefix first, equal
                                        sequences in input order) and a row is dropped when the row before it in that order has the
                                        same sequence and the same x.5 flag.  Only the groups' row numbers and the answer cross the
                                        link; n_tie_rows / n_tie_dropped are filled as with the callback.  A group row without a
                                        sequence fails the call with CSV_E_INVALID; the context stays usable */
};
/* The rows of the keep-every-row segments (seg_nodedup) whose integer keys tie - (segment, a, b, read_id) equal - are ordered
 * by data only the caller has: the reference sorts INS rows by (chr, int(pos), len, read, SEQUENCE) and drops a row only when
 * the whole tuple repeats, the x.5 of a split-read position included (MAIN:774-775, :958-969).  csv_rebuild_signatures sorts on
 * the integer columns on the device, hands the tie groups - a few rows per genome - to this function ONCE, on the calling
 * thread, and applies the answer to the device-resident permutation before the rows are gathered: the columns never come to
 * the host for it (CSV_RB_KEEP_ON_DEVICE -> CSV_IN_DEVICE_COLUMNS stays intact).
 *   rows [group_off[g], group_off[g + 1]) of src_row are group g, in the device's stable order (= input order);
 *   order[i]  the callee's position of row i INSIDE its group (a permutation of 0 .. size - 1 per group),
 *   drop[i]   1: the row is a duplicate and is removed.
 * Return 0; anything else fails the call with CSV_E_INVALID. */
typedef int (*csv_tie_order_fn)(void* user, int64_t n_groups, const int64_t* group_off, const int32_t* src_row, int32_t* order, uint8_t* drop);

typedef struct csv_rebuild_in {
    int64_t        n;
    int32_t        n_seg;
    int32_t        flags;           /* CSV_RB_* */
    const uint8_t* seg_aux_major;   /* n_seg */
    const int32_t* seg_id;
    const int64_t* a;
    const int64_t* b;
    const int32_t* read_id;
    const int32_t* aux;
    const uint8_t* seg_nodedup;     /* n_seg or NULL: 1 = sort this segment but keep every row.  INS rows are equal only when
                                       their sequences and the x.5 of a split-read position are equal too (MAIN:228, :774-775):
                                       tie_order (below) settles those few groups; without it the caller finishes them on the host */
    const int32_t* read_rank;       /* CSV_RB_FROM_POOL: n_rank ranks, indexed by the pool rows' read index */
    int64_t        n_rank;
    csv_tie_order_fn tie_order;     /* nullable (ABI v6): see csv_tie_order_fn */
    void*          tie_user;
} csv_rebuild_in;

typedef struct csv_rebuild_out {
    int64_t  n_out;                 /* out */
    int32_t* seg_id;
    int64_t* a;
    int64_t* b;
    int32_t* read_id;
    int32_t* aux;
    int32_t* src_row;
    float    ms_device;             /* out: kernels only (HIP events) */
    int32_t  n_passes;              /* out: radix passes executed */
    int64_t* seg_count;             /* n_seg or NULL: rows of every segment after the de-duplication (the csv_segment ranges of the
                                       sorted columns follow from these by a prefix sum) */
    int64_t  n_ins_ties;            /* out: rows of seg_nodedup segments that agree with their predecessor in (segment, a, b, read_id) and
                                       were NOT settled by tie_order: 0 means the device order is final, otherwise (no tie_order given)
                                       the caller finishes those groups on the host */
    void*    dev_seg_id;            /* out (CSV_RB_KEEP_ON_DEVICE): device addresses of the sorted columns, n_out rows each: */
    void*    dev_a;                 /*   int32 seg_id, int64 a, int64 b, int32 read_id, int32 aux, int32 src_row */
    void*    dev_b;
    void*    dev_read_id;
    void*    dev_aux;
    void*    dev_src_row;
    int64_t  n_tie_rows;            /* out (ABI v6): rows handed to tie_order, and how many of them it dropped */
    int64_t  n_tie_dropped;
} csv_rebuild_out;

int csv_rebuild_signatures(csv_ctx* ctx, const csv_rebuild_in* in, csv_rebuild_out* out);
/* Which sort the context's last successful csv_rebuild_signatures took (chosen per call from the widths of the key columns):
 * 1 = composite key in 16-byte elements, 2 = composite key in 32-byte elements, 3 = the permutation sort (keys beyond 128 bits,
 * or CSV_RB_PERM_SORT set); 0 = no rebuild has sorted anything on this context yet (a call with no rows does not count). */
int csv_rebuild_route(const csv_ctx* ctx);

/* The device-resident signature pool: the reference's dataflow extraction -> rebuild (MAIN:697-743 -> 750-857) without a trip
 * through host memory.  csv_cigar_signatures with CSV_CG_TO_POOL appends the signatures it finds as rows (segment, position,
 * length, global read index, aux), csv_split_signatures its candidates; csv_pool_append adds rows the host made;
 * csv_rebuild_signatures with CSV_RB_FROM_POOL sorts and de-duplicates the pool.  The pool belongs to the context and
 * lives until csv_pool_reset / csv_ctx_destroy. */
int csv_pool_reset(csv_ctx* ctx);
int csv_pool_rows(const csv_ctx* ctx, int64_t* n_rows);
int csv_pool_append(csv_ctx* ctx, int64_t n, const int32_t* seg_id, const int64_t* a, const int64_t* b, const int32_t* read, const int32_t* aux);

/* The device-resident name pool: the read names behind the pool rows' read indices, and their ranks (names.hip.h, DESIGN.md
 * section 15).  The rebuild order ends in the read name (MAIN:764-802: rows that tie on (pos, len) order by name; :958-969: a row
 * repeats when its name repeats too), so the read-id column of the sorted rows must be an integer whose order is the names'
 * string order.  A caller appends the names of every chunk it extracts - name index = the read index its pool rows carry - and
 * CSV_RB_RANK_FROM_NAMES makes the rebuild use their ranks: no name is sorted, hashed or looked up on the host.
 *
 * csv_name_pool_append: name i of the call = bytes[off[i] .. off[i] + len[i]); the names get the indices first_index ..
 *   first_index + n - 1.  The strided form is exactly a csv_bam_chunk's host image: bytes = host, off = host_off, len =
 *   l_read_name - 1.  Every [off, off + len) is checked against n_bytes and 0 <= len <= 255 on the host before anything is
 *   launched: CSV_E_INVALID otherwise, and the pool is unchanged.  The names are kept compact in a grow-only arena of the
 *   context (a blob plus offsets); the pool lives until csv_name_pool_reset / csv_ctx_destroy.
 * csv_name_ranks: rank[i] = index of name i in sorted(set(names)), the names compared as unsigned bytes - a name that is a prefix
 *   of another sorts first, equal names get equal ranks; for ASCII names this is Python's str order.  first[r] = the smallest
 *   index that holds the name of rank r (n_distinct entries; CSV_E_CAPACITY when cap_first is smaller, n_distinct holds the
 *   need).  `rank` (n entries, n = csv_name_pool_rows) and `first` may be NULL.  The ranks stay in device memory (dev_rank, int32,
 *   valid until the next append / reset) and are cached: a second call without an append in between launches nothing and
 *   reports the figures of the run that made them.  n_passes: radix passes executed = byte positions at which any two names
 *   differ (names that share a prefix or have fixed separators cost nothing there); max_len: the longest name.
 * csv_name_pool_get: the names at index[0 .. n) gathered into one blob on the device and downloaded: name k = out[out_off[k] ..
 *   out_off[k + 1]), no terminator.  Turns ids back into text (support lists, --report_readid: GT:263-458), typically for the
 *   names at first[...] of the few thousand reads that support calls.  CSV_E_CAPACITY: cap is too small, out_off[n] holds the
 *   need.  CSV_E_INVALID: an index outside the pool. */
typedef struct csv_name_rank_out {
    int64_t  n;                     /* out: names in the pool */
    int64_t  n_distinct;            /* out */
    int32_t* rank;                  /* n or NULL */
    int32_t* first;                 /* cap_first or NULL */
    int64_t  cap_first;
    float    ms_device;             /* out: kernels only (HIP events) */
    int32_t  n_passes;              /* out */
    int32_t  max_len;               /* out */
    int32_t  reserved;
    void*    dev_rank;              /* out: int32 ranks in device memory, n entries */
} csv_name_rank_out;

int csv_name_pool_reset(csv_ctx* ctx);
int csv_name_pool_rows(const csv_ctx* ctx, int64_t* n);
int csv_name_pool_append(csv_ctx* ctx, int64_t n, const uint8_t* bytes, int64_t n_bytes, const int64_t* off, const int32_t* len, int64_t* first_index);
int csv_name_ranks(csv_ctx* ctx, csv_name_rank_out* out);
int csv_name_pool_get(csv_ctx* ctx, int64_t n, const int32_t* index, char* out, int64_t cap, int64_t* out_off /* n + 1 */);
/* sizeof of 0 csv_name_rank_out; 0 otherwise */
size_t csv_name_struct_size(int which);

/* The device-resident INS sequence pool (seqs.hip.h): beside every INS row of the signature pool its
 * inserted bases (ASCII) and the x.5 flag of a split-read position - the fourth element of the reference's INS tuple (MAIN:537,
 * :639-640, :228) - made where the rows are made, compared there for the rebuild (CSV_RB_TIES_FROM_SEQS) and returned by pool row.
 *
 * csv_seq_reads_upload: the sequences of the current batch's reads in the BAM 4-bit encoding - read i = (l_seq[i] + 1) / 2 bytes
 *   at bytes + off[i], high nibble first, code -> "=ACMGRSVTWYHKDBN".  This is the strided form of a csv_bam_chunk's host image
 *   (bytes = host, off = host_off + l_read_name).  want: n_reads bytes or NULL; want[i] = 0: read i's bases are not needed and
 *   not sent.  Every range is checked against n_bytes before anything is launched (CSV_E_INVALID, state unchanged).  The wanted
 *   reads are packed back to back on the host and cross the link once.  Index space: the batch's read index (what is added to
 *   read_base).  The bases live in a buffer of their own until the next upload or the next csv_bam_decode.
 * csv_seq_query_reverse: for a csv_split_signatures call WITHOUT CSV_SP_FROM_BAM, per read of the last upload 1 when the record's
 *   flag is 16 - the query parse_read hands on is then the reverse complement of the stored sequence (MAIN:673-675).
 * CSV_CG_SEQ_TO_POOL (csv_cigar_in.flags and csv_split_in.flags, only with CSV_CG_TO_POOL): the INS rows the call appends get
 *   their bases.  CIGAR scan: the pieces query[qoff : qoff + len], each clipped to the read like a Python slice, concatenated.
 *   Split analysis (kind 1): q[c:d], clipped likewise, q = the stored sequence (flag != 16) or its reverse complement (flag == 16;
 *   CSV_SP_FROM_BAM: the decode's flag of the call's record), reverse-complemented once more when aux bit 0 is set; the
 *   complement is A <-> T, C <-> G, everything else unchanged; x.5 flag = aux bit 1 AND the low bit of a.  The length of a row's
 *   bases equals its aux (query_len, when given, must be the uploaded l_seq; NULL in csv_cigar_in: l_seq is used).  A row whose
 *   read has no uploaded sequence, a negative slice bound or a length that is not the row's aux fails the call with
 *   CSV_E_INVALID: the pool and the sequence pool keep their row counts.
 * csv_seq_pool_rows: INS rows that hold a sequence, bytes of the blob.  csv_pool_reset empties the sequence pool, too.
 * csv_seq_pool_put: host-made ASCII sequences for EXISTING pool rows (the INS rows a caller appended with csv_pool_append):
 *   sequence k = bytes[off[k] .. off[k] + len[k]), half[k] (NULL: 0) its x.5 flag.  A row out of range, named twice or with a
 *   sequence already, or len[k] != the row's aux: CSV_E_INVALID and nothing changes.
 * csv_seq_pool_get: the bases of pool_row[0 .. n) gathered into one blob on the device (one wavefront per row) and downloaded:
 *   row k = out[out_off[k] .. out_off[k + 1]).  CSV_E_CAPACITY: cap is too small, out_off[n] holds the need.  CSV_E_INVALID: a row
 *   out of range or without a sequence.  csv_seq_pool_half: the rows' x.5 flags (0 for a row without a sequence). */
typedef struct csv_seq_info {
    int64_t reads_uploaded;         /* of the last csv_seq_reads_upload: wanted reads, bytes that crossed the link */
    int64_t bytes_uploaded;
    int64_t rows_gathered;          /* of the last CSV_CG_SEQ_TO_POOL call: rows that got bases, their bytes */
    int64_t bytes_gathered;
    float   ms_upload;              /* host wall time of the last upload: packing, copies, wait */
    float   ms_gather;              /* kernels of the last CSV_CG_SEQ_TO_POOL call: lengths, scan, gather (HIP events) */
    int32_t packed;                 /* 1: the wanted reads were packed before the copy */
    int32_t reserved;
    int64_t device_bytes;           /* device memory the sequence pool holds now: uploaded reads, blob, row arrays, per-call scratch */
} csv_seq_info;

int csv_seq_reads_upload(csv_ctx* ctx, int64_t n_reads, const uint8_t* bytes, int64_t n_bytes, const int64_t* off, const int32_t* l_seq, const uint8_t* want);
/* CSV_SEQ_OPT_WHOLE_IMAGE (a measurement aid, per context, default 0): value 1 makes csv_seq_reads_upload send `bytes` whole instead of
 * packing the wanted reads first - the form scripts/ins_seq_stage.py times against the packed one; results are
 * the same either way. */
enum { CSV_SEQ_OPT_WHOLE_IMAGE = 1 };
int csv_seq_option(csv_ctx* ctx, int which, int value);
int csv_seq_query_reverse(csv_ctx* ctx, int64_t n_reads, const uint8_t* reverse);
int csv_seq_pool_rows(const csv_ctx* ctx, int64_t* n_with_seq, int64_t* n_bytes);
int csv_seq_pool_put(csv_ctx* ctx, int64_t n, const int32_t* pool_row, const uint8_t* bytes, int64_t n_bytes, const int64_t* off, const int32_t* len, const uint8_t* half);
int csv_seq_pool_get(csv_ctx* ctx, int64_t n, const int32_t* pool_row, char* out, int64_t cap, int64_t* out_off /* n + 1 */);
int csv_seq_pool_half(csv_ctx* ctx, int64_t n, const int32_t* pool_row, uint8_t* half);
int csv_seq_info_get(const csv_ctx* ctx, csv_seq_info* out);
/* sizeof of 0 csv_seq_info; -1 past the end */
int csv_seq_struct_size(int which);

/* The two strings a VCF record takes from the pools, gathered on the device (vcf_strings.hip.h).  Both
 * read the sorted columns of the context's last KEPT pool rebuild - csv_rebuild_signatures with CSV_RB_FROM_POOL |
 * CSV_RB_KEEP_ON_DEVICE: dev_src_row, dev_read_id, dev_aux, n_out rows - and produce the CSR blobs csv_vcf_in takes.  They
 * return CSV_E_INVALID and launch nothing when the context holds no such rebuild, or when csv_pool_reset, csv_pool_append,
 * csv_name_pool_reset, csv_name_pool_append, another csv_rebuild_signatures, csv_cigar_signatures or csv_split_signatures was
 * called since (the columns and the pools no longer belong together: rebuild again).  csv_cluster_batch on those columns
 * (CSV_IN_DEVICE_COLUMNS) changes nothing.  After any failure the context stays usable and the pools are unchanged.
 *
 * csv_seq_alt_gather: entry k = bases(pool row dev_src_row[pick[k]])[0 .. clip[k]) - the ALT of an INS call whose seq_pick is
 *   pick[k] and whose SVLEN (bp2) is clip[k] (cuteSV_resolveINDEL.py:402); its length is min(aux, clip).  pick and clip are
 *   int64_t arrays, or int32_t arrays with flags = CSV_OUT_COORD_I32 (the seq_pick / bp2 of such a result).  CSV_E_INVALID, with
 *   nothing written to `out`: a pick outside [0, n_out), a clip < 0 (the reference has none, and a Python slice would count
 *   from the end), a picked row without a sequence.  out_off (n + 1 entries) is filled first; CSV_E_CAPACITY: cap is too
 *   small, out_off[n] holds the need.
 * csv_name_support_join: entry c = the names of the reads first[dev_read_id[s]], s = support[support_off[c] ..
 *   support_off[c + 1]), joined with ',' in the order of the list - the RNAMES text of cuteSV_genotype.py:263-458; a call
 *   without supports is an empty entry.  The support list is support_sig (int64_t) or support_sig32 (int32_t), the other
 *   NULL, as in csv_batch_out.  Needs a rebuild made with CSV_RB_RANK_FROM_NAMES (CSV_E_INVALID otherwise); a support
 *   outside [0, n_out) or offsets that do not start at 0 or decrease: CSV_E_INVALID.  out_off (n_calls + 1 entries) and
 *   CSV_E_CAPACITY as above. */
int csv_seq_alt_gather(csv_ctx* ctx, int64_t n, const void* pick, const void* clip, int32_t flags, char* out, int64_t cap, int64_t* out_off /* n + 1 */);
int csv_name_support_join(csv_ctx* ctx, int64_t n_calls, const int64_t* support_off /* n_calls + 1 */, const int64_t* support_sig, const int32_t* support_sig32, char* out,
                          int64_t cap, int64_t* out_off /* n_calls + 1 */);

/* The text signature files of cuteSV's --write_old_sigs (main script :763-808) from the same kept rebuild (vcf_strings.hip.h,
 * DESIGN.md section 24): rows [row_begin, row_end) of its sorted columns - dev_seg_id, dev_a, dev_b, dev_read_id, dev_aux,
 * dev_src_row - become one line each, back to back in `out`.  Segment s has type {DEL, INS, INV, DUP, TRA}[s / n_chrom] and
 * chromosome s % n_chrom of the caller's table: chromosome k's name = chrom_names[chrom_off[k] .. chrom_off[k + 1]), in name-rank
 * order (the numbering of a TRA row's mate too).
 *   DEL / DUP   TYPE \t chr \t a \t b \t read \n
 *   INS         TYPE \t chr \t a \t b \t read \t bases \n              bases = the sequence-pool entry of pool row dev_src_row (aux bytes)
 *   INV         TYPE \t chr \t strand \t a \t b \t read \n            strand = strand0 / strand1 for aux 0 / 1 (at most 15 bytes each)
 *   TRA         TYPE \t chr \t A|B|C|D \t a \t chr2 \t b \t read \n    type = aux & 7, chr2 = chromosome aux >> 3
 * read = the name first[dev_read_id] of the name pool (the rebuild must have been made with CSV_RB_RANK_FROM_NAMES); a and b in
 * decimal.  *need receives the bytes of the lines whenever the rows are in order; CSV_E_CAPACITY: cap is smaller, nothing is
 * stored.  CSV_E_INVALID, with nothing stored: no kept rebuild or the pools changed since (as above), a row range outside
 * [0, n_out], a malformed table, and any row with a or b outside [0, 2^42), a read id outside the name pool's ranks, an INS row
 * without a sequence, a TRA type above 3 or a mate outside the table, an INV strand code above 1, a segment outside
 * 5 * n_chrom; also more than 2^31 - 4096 bytes in one call (ask for fewer rows).  ms_kernels (may be NULL): the kernels' time
 * from HIP events. */
int csv_pool_sigs_text(csv_ctx* ctx, int64_t row_begin, int64_t row_end, const char* chrom_names, const int64_t* chrom_off /* n_chrom + 1 */, int32_t n_chrom,
                       const char* strand0, const char* strand1, char* out, int64_t cap, int64_t* need, float* ms_kernels);

/* The alignment table and the TRA genotyping over it (aln.hip.h).  The reference genotypes a TRA call from
 * the BAM itself (call_gt, cuteSV_resolveTRA.py:258-309; count_coverage, cuteSV_genotype.py:72-93): every alignment fetch()
 * yields counts - secondary, supplementary, low-MAPQ and placed-unmapped records too - and a record is primary when its flag is
 * 0 or 16, whatever its MAPQ.  The table holds one row per BAM record, grouped by chromosome, in file order:
 *   start    pos
 *   end      pos + max(reference span, 1); pos + 1 for a record without CIGAR, with a zero span or with flag bit 4 (htslib's
 *            bam_endpos); a CG-tag record takes its span from the CG array; saturates at INT32_MAX
 *   primary  flag == 0 || flag == 16
 *   id       the name id of the record
 * (12 bytes per record in device memory), and per chromosome the longest end - start.  It belongs to the context and lives
 * until csv_aln_reset / csv_ctx_destroy.
 *
 * csv_aln_reset: empties the table and fixes the number of chromosomes.  csv_aln_rows: its row count.
 * csv_aln_append_decoded: the records of the context's last successful csv_bam_decode (CSV_E_INVALID: there is none) with
 *   beg <= pos < end become rows of `chrom`, in chunk order, each with the name id name_base + its index in the chunk - the
 *   reference_start >= task start rule of the reads table (MAIN:711): tasks partition a contig, so every record lands in the
 *   table once.  Filter, scan, compaction and conversion run on the device; nothing but the count comes back.
 * csv_aln_append: the same from host arrays (0 <= start < end, id >= 0: CSV_E_INVALID otherwise).
 * Ordering contract of both: chrom must be at least the chromosome of the last row, and the starts must not decrease inside a
 *   chromosome, across appends too: CSV_E_UNSORTED.  A chrom outside [0, n_chrom): CSV_E_INVALID.  The order of the starts is
 *   checked on the device (a flag word that comes back with the count).  After a failed append the table is unchanged.
 * csv_aln_get: rows [first, first + n) back to the host (any array may be NULL).  csv_aln_layout: off[n_chrom + 1] = first row of
 *   every chromosome, maxlen[n_chrom] = its longest record (0: no rows).  csv_aln_timing: the kernels of the last append / the last
 *   genotype call in milliseconds (HIP events).
 * csv_aln_tra_genotype: call_gt for n_calls calls, one wavefront each.  Window 1 = [max(pos1 - bias, 0), min(pos1 + bias,
 *   contig_len[chrom1])); count_coverage's walk over the rows with start < e and end > s, with its two exits - A: the row is
 *   primary, starts before s, ends after e, and the distinct names of such rows reach up_bound -> 1; B: the row is primary and
 *   it is at least the gt_round-th of the walk -> 1 when 5 * primaries <= rows so far, else -1.  Window 2 (pos2 on chrom2) is
 *   walked only when window 1 gave 0, and its status is not looked at.  out_status = window 1's status; out_dr = the spanning
 *   names that are not among the call's supports, -1 when the status is -1.  up_bound = threshold_ref_count
 *   (cuteSV_genotype.py:62-70) of the call's support count.  A window that is empty after the clamp walks nothing.
 *   support: int64_t, or int32_t with CSV_ALN_SUPPORT_I32.  Without CSV_ALN_FROM_KEPT_REBUILD it holds ids (>= 0), compared with
 *   the rows' ids as they are.  With it, it holds rows of the context's last kept pool rebuild (the support_sig of a result),
 *   under the contract of csv_name_support_join: a support's id is dev_read_id[row], a name rank; a table row's id is the rank
 *   of its name id in the name pool, whose ranks must be current - both looked up on the device.
 *   CSV_E_INVALID, with nothing launched and the context usable: offsets that do not start at 0 or decrease, a support outside
 *   its range, a chromosome outside [0, n_chrom), n_chrom that is not the table's, in rank mode a name id of the table outside
 *   the name pool, no kept rebuild by name, or pools that changed since. */
enum { CSV_ALN_FROM_KEPT_REBUILD = 1, CSV_ALN_SUPPORT_I32 = 2 };
int csv_aln_reset(csv_ctx* ctx, int32_t n_chrom);
int csv_aln_rows(const csv_ctx* ctx, int64_t* n);
int csv_aln_append_decoded(csv_ctx* ctx, int32_t chrom, int64_t beg, int64_t end, int64_t name_base, int64_t* n_appended);
int csv_aln_append(csv_ctx* ctx, int32_t chrom, int64_t n, const int32_t* start, const int32_t* end, const uint8_t* primary, const int32_t* id);
int csv_aln_get(csv_ctx* ctx, int64_t first, int64_t n, int32_t* start, int32_t* end, uint8_t* primary, int32_t* id);
int csv_aln_layout(csv_ctx* ctx, int32_t n_chrom, int64_t* off /* n_chrom + 1 */, int32_t* maxlen /* n_chrom */);
int csv_aln_timing(const csv_ctx* ctx, float* ms_append, float* ms_genotype);
int csv_aln_tra_genotype(csv_ctx* ctx, int64_t n_calls, const int32_t* chrom1, const int64_t* pos1, const int32_t* chrom2, const int64_t* pos2,
                         const int64_t* support_off /* n_calls + 1 */, const void* support, int32_t flags, int32_t n_chrom, const int64_t* contig_len, int64_t bias,
                         int64_t gt_round, int32_t* out_dr, int32_t* out_status);

/* ---------------------------------------------------------------------------------------------
 * The CIGAR scan of the extraction step on the GPU.  Restates the CIGAR part of parse_read
 * (cuteSV main script :606-655: every I / D operation of at least min_siglength bases is a piece at the reference position
 * it is reached, :629-643) and generate_combine_sigs (:515-575: pieces of one type within merge_ins_threshold /
 * merge_del_threshold of each other inside a read become one signature; the distance rule of :535 / :558 / :569 is
 * reproduced as written).  BAM decode and the bases stay in the Python driver with pysam (the SA-tag split-read analysis
 * is csv_split_signatures below): the input is the flat BAM-encoded CIGAR array of a batch of reads (pysam: read.cigartuples), the output the
 * INS / DEL signatures in read order plus, for INS, the query slices the inserted sequence is made of
 * (query_sequence[qoff : qoff + len] per piece, concatenated: :639-640, :537).
 *   use[r] = 0 skips read r (mapq < min_mapq, :614; the query_length < min_read_len gate of :607 is the caller's too).
 * Outputs are caller-allocated; CSV_E_CAPACITY fills n_sig_ins / n_piece_ins / n_sig_del with the need.
 */
typedef struct csv_cigar_in {
    int64_t         n_reads;
    const int64_t*  cig_off;        /* n_reads + 1 offsets into cigar */
    const uint32_t* cigar;          /* oplen << 4 | op, op = 0..9 for M I D N S H P = X B (the BAM encoding) */
    const int64_t*  ref_start;      /* read.reference_start, 0-based */
    const uint8_t*  use;            /* n_reads or NULL */
    int32_t         min_siglength;  /* --min_siglength (cuteSV_Description.py:152) */
    int32_t         flags;          /* CSV_CG_* */
    int64_t         merge_ins_threshold;   /* --merge_ins_threshold (:127) */
    int64_t         merge_del_threshold;   /* --merge_del_threshold (:123) */
    /* CSV_CG_TO_POOL: the signatures also become rows of the context's pool - INS rows in segment seg_ins, DEL rows in seg_del
     * (the caller's numbering of (chromosome, type)), read index = read_base + the read's index in this batch, aux of an INS
     * row = length of the sequence the caller would cut out of the read (the pieces clipped to query_len[read] like Python
     * slices; query_len NULL: the signature's length).  Output arrays of csv_cigar_out that are NULL are then not written
     * (their capacities still bound the counts). */
    int32_t         seg_ins, seg_del;
    int64_t         read_base;
    const int32_t*  query_len;      /* n_reads or NULL */
} csv_cigar_in;
enum { CSV_CG_TO_POOL = 1,
       /* cig_off, cigar and ref_start are NOT read from `in`: they are the device columns the context's last csv_bam_decode
        * made (n_reads must be its record count).  `use` is still the caller's host array (or CSV_CG_USE_FROM_GATES).  The CIGARs never cross PCIe. */
       CSV_CG_FROM_BAM = 2,
       /* only with CSV_CG_TO_POOL, in csv_cigar_in.flags and csv_split_in.flags alike (there 4 is CSV_SP_FROM_BAM): the INS rows'
        * bases go to the context's sequence pool (csv_seq_* above) */
       CSV_CG_SEQ_TO_POOL = 8,
       /* only with CSV_CG_FROM_BAM and use == NULL: use[r] is bit CSV_GATE_USE of the gates csv_bam_task_gates left in device memory
        * beside that decode.  CSV_E_INVALID, nothing launched: CSV_CG_FROM_BAM is missing, `use` is given as well, or the context
        * holds no gates of its last csv_bam_decode. */
       CSV_CG_USE_FROM_GATES = 16 };

typedef struct csv_cigar_out {
    int64_t  cap_sig_ins, cap_piece_ins, cap_sig_del;
    int64_t  n_sig_ins, n_piece_ins, n_sig_del;          /* out */
    int32_t* ins_read;  int64_t* ins_pos;  int64_t* ins_len;  int64_t* ins_piece0;  int32_t* ins_npiece;     /* cap_sig_ins */
    int32_t* piece_qoff;  int32_t* piece_len;                                                               /* cap_piece_ins */
    int32_t* del_read;  int64_t* del_pos;  int64_t* del_len;                                                /* cap_sig_del */
    float    ms_device;                                  /* out: kernels only (HIP events) */
    int32_t  reserved;
} csv_cigar_out;

int csv_cigar_signatures(csv_ctx* ctx, const csv_cigar_in* in, csv_cigar_out* out);

/* ---------------------------------------------------------------------------------------------
 * The split-read analysis of the extraction step on the GPU (second half).  Restates
 * organize_split_signal (cuteSV main script :483-513: the primary alignment plus the SA-tag entries that pass min_mapq
 * become [read_start, read_end, ref_start, ref_end, chr, strand] segments; reads with more than max_split_parts segments
 * are skipped) and analysis_split_read with analysis_inv / analysis_bnd (:50-464: segments sorted by read_start, then
 * the two-segment and sliding three-segment rules that emit INV / TRA / DUP / INS / DEL candidates).  The input is
 * numbers, not text: per entry what acquire_clip_pos (:466-481) takes out of the SA entry's CIGAR and the numbers of the
 * entry itself.  A caller with pysam records makes them from the tag's text (extract.encode_split_reads); for a chunk of
 * the native BAM reader csv_bam_split_inputs makes them on the device and CSV_SP_FROM_BAM uses them where they are.
 *
 * Entries of read r: [ent_off[r], ent_off[r + 1]), the primary alignment first when the read has one (parse_read
 * :660-668, primary = 1: c0/c1 = read_start/read_end, f0/f1 = ref_start/ref_end as parse_read computes them), then the
 * SA entries in tag order (primary = 0: c0/c1 = leading / trailing soft-clip lengths, f0 = 0-based start, f1 = reference
 * span, mapq).  chr is an integer whose order is the Python string order of the chromosome names (analysis_bnd compares
 * names with <, :110).  strand: 0 '+', 1 '-'.
 *
 * Output: one record per candidate, reads in order, inside a read in the order the reference appends them (per SV type
 * that is exactly the order of the reference's five lists).  kind: 0 DEL (a = pos, b = length), 1 INS (a = position
 * numerator, b = length, c / d = the Python slice bounds query[c:d] of the inserted sequence, aux bit 0: the slice is
 * taken from the reverse complement of the query analysis_split_read was given, aux bit 1: the position is the float
 * a / 2 (:228, :244) rather than the integer a (:452)), 2 DUP (a, b = the two positions), 3 INV (aux: 0 "++", 1 "--";
 * a, b), 4 TRA (aux: 0..3 = 'A'..'D'; a = pos1, c = mate chromosome, b = pos2).  chr = the tuple's last element.
 */
typedef struct csv_split_in {
    int64_t         n_reads;
    const int64_t*  ent_off;        /* n_reads + 1 */
    const int64_t*  read_len;       /* read.query_length (total_L / RLength) */
    const int64_t*  c0;  const int64_t* c1;  const int64_t* f0;  const int64_t* f1;      /* per entry */
    const int32_t*  chr; const int32_t* mapq;
    const uint8_t*  strand;  const uint8_t* primary;
    int64_t         sv_size;        /* --min_size (parse_read's SV_size) */
    int64_t         max_size;       /* --max_size, -1: no limit */
    int32_t         min_mapq;
    int32_t         max_split_parts;   /* -1: no limit */
    /* CSV_CG_TO_POOL in `flags`: the candidates also become rows of the context's pool (csv_pool_* above).  A candidate of kind k
     * (0 DEL, 1 INS, 2 DUP, 3 INV, 4 TRA) on chromosome rank ch goes to segment pool_seg_base[k] + ch with the columns the rebuild
     * sorts on: (pos, len) for DEL / INS (an x.5 INS position as its integer part; aux = length of query[c:d], clipped to
     * query_len[read] - NULL: read_len - like a Python slice), (pos1, pos2) for DUP, aux = strand code for INV, aux = chr2 * 8 +
     * type for TRA; read index = read_base + the read's index in this batch.  Output arrays of csv_split_out that are NULL are
     * then not written. */
    int32_t         flags;          /* CSV_CG_TO_POOL, CSV_SP_FROM_BAM, CSV_CG_SEQ_TO_POOL */
    int32_t         pool_seg_base[5];
    int64_t         read_base;
    const int32_t*  query_len;      /* n_reads or NULL */
} csv_split_in;
/* csv_split_in.flags, next to CSV_CG_TO_POOL = 1: n_reads, ent_off, read_len and the eight entry columns are NOT read from
 * `in`: the reads are the calls of the context's last csv_bam_split_inputs and the columns are the ones it left on the
 * device (CSV_E_INVALID when the context holds none).  A call it flagged has no entries and yields nothing.  out->read is
 * the call index.  With CSV_CG_TO_POOL a row's read index is read_base + call_rec[call] - the record's index in the
 * chunk, the index space of the CIGAR scan's rows of that chunk - and the query length is the decode's column: the
 * query_len pointer of `in` is ignored. */
enum { CSV_SP_FROM_BAM = 4 };

typedef struct csv_split_out {
    int64_t  cap;
    int64_t  n;                     /* out */
    uint8_t* kind;  int32_t* read;  int32_t* chr;  int32_t* aux;  int64_t* a;  int64_t* b;  int64_t* c;  int64_t* d;   /* cap */
    float    ms_device;             /* out: kernels only */
    int32_t  reserved;
} csv_split_out;

int csv_split_signatures(csv_ctx* ctx, const csv_split_in* in, csv_split_out* out);

/* ---------------------------------------------------------------------------------------------
 * Host-side VCF record emit: the structure-of-arrays result -> the text lines
 * of cuteSV's VCF body, without materialising Python row lists.  Replaces generate_output
 * (cuteSV_genotype.py:242-467: per-chromosome stable sort by POS, size filters, INFO/FORMAT
 * assembly, REF/ALT from the reference sequence, q5 filter, AF) and the SVID numbering of main_ctrl
 * (cuteSV main script :1208-1237: one counter per SV type over the sorted chromosome names).
 * No GPU work: plain C++ on the caller's thread.
 */
typedef struct csv_vcf_in {
    /* the calls (csv_batch_out after csv_cluster_batch / csv_batch_download) and their segments */
    const csv_batch_out* res;
    const csv_segment*   seg;
    int32_t              n_seg;
    int32_t              n_chrom;
    /* per chromosome (index = csv_segment.chrom): name, reference sequence, emission rank
     * (chrom_rank[c] = position of chromosome c in sorted(names): the order main_ctrl writes them) */
    const char* const*   chrom_name;
    const char* const*   chrom_seq;
    const int64_t*       chrom_len;
    const int32_t*       chrom_rank;
    /* strings attached to calls, as CSR blobs indexed by call (NULL = absent):
     *   ins_alt  the inserted sequence already sliced to SVLEN (INS calls; INDEL:402)
     *   rnames   comma-joined supporting read names (only read when report_readid)            */
    const char*          ins_alt;    const int64_t* ins_alt_off;
    const char*          rnames;     const int64_t* rnames_off;
    /* INV strand strings by call_aux code; genotype strings by table row:
     *   gl_key[n_gl] sorted gl_idx values present, gl_str = per key "GT\tPL\tGQ\tQUAL" (tab separated) */
    const char* const*   strand_name;
    const int32_t*       gl_key;     const char* const* gl_str;     int32_t n_gl;
    /* flags of cuteSV_Description.py: --min_size (:144), --max_size (:148), --genotype (:159), --report_readid (:100), --ignore_sequence (:104) */
    int64_t              min_size;
    int64_t              max_size;
    int32_t              genotype;
    int32_t              report_readid;
    int32_t              ignore_sequence;
    int32_t              reserved;
    /* (ABI v6) chrom_seq[c] may point INTO a FASTA file (mmap) instead of at a contiguous string: per chromosome the bases per
     * line and the bytes per line (bases + line break) of its `.fai` entry; NULL arrays or a 0 entry = contiguous */
    const int32_t*       chrom_line_bases;
    const int32_t*       chrom_line_width;
} csv_vcf_in;

/* Writes the records into `out` (capacity `cap` bytes) and returns CSV_OK, or CSV_E_CAPACITY with
 * *n_written = the needed size.  svid[5] = running record counters in the order INS, DEL, BND, DUP, INV
 * (main script :1209-1213); pass zeros for a fresh file, they are advanced in place. */
int csv_vcf_emit(const csv_vcf_in* in, char* out, int64_t cap, int64_t* n_written, int64_t* svid);

/* The `.fai` of a FASTA file held in memory (e.g. mmap): what pysam.FastaFile / `samtools faidx` give generate_output
 * (GT:254-259) - per contig its name (name_off / name_len address the header text inside `data`, up to the first white space),
 * length, byte offset of the first base, bases per line and bytes per line.  Returns the number of contigs found (call again
 * with larger arrays when it exceeds max_contigs; NULL arrays are skipped), or -CSV_E_INVALID for a file that cannot
 * be indexed (sequence before a header, lines of unequal length inside a contig).  No GPU work. */
int64_t csv_fasta_index(const char* data, int64_t size, int64_t max_contigs, int64_t* name_off, int32_t* name_len,
                        int64_t* length, int64_t* offset, int32_t* line_bases, int32_t* line_width);

/* csv_fasta_index for a text that is never in memory whole (a BGZF-compressed FASTA inflated window by window):
 * open, feed the windows in order, finish, close.  For every cut of a text into windows the entries and the verdict are those of
 * csv_fasta_index over the whole text.  feed: CSV_OK, or CSV_E_INVALID from the first refusal on.  finish: the number of contigs
 * or -CSV_E_INVALID; the arrays receive the first max_contigs entries, *names_bytes the bytes of all names, `names` those bytes back
 * to back when they fit names_cap (name_off addresses them there).  finish may be called again with larger arrays.  No GPU work. */
typedef struct csv_fai_stream csv_fai_stream;
csv_fai_stream* csv_fasta_index_stream_open(void);
int csv_fasta_index_stream_feed(csv_fai_stream* s, const char* data, int64_t size);
int64_t csv_fasta_index_stream_finish(csv_fai_stream* s, int64_t max_contigs, char* names, int64_t names_cap, int64_t* names_bytes, int64_t* name_off,
                                      int32_t* name_len, int64_t* length, int64_t* offset, int32_t* line_bases, int32_t* line_width);
void csv_fasta_index_stream_close(csv_fai_stream* s);
/* A window may also be fed as its event rows (csrc/ref_core.h; csv_fai_events below makes them on the device, csv_fai_events_host on
 * the host), in any mix with windows fed as bytes.  carry: carry[3] <- the line in progress (its absolute first byte, that byte, the
 * last byte seen), which the rows of the next window are made with.  rows: the next window, window_bytes long, as n_rows rows of 3
 * int64 {absolute first byte of a line, its bytes without the line break, its bases | 1 << 62 for a header}, the header texts and the
 * carry behind the window, as csv_fai_events gave them.  CSV_E_INVALID: the text is refused, or the rows do not describe a window
 * behind the text fed so far. */
int csv_fasta_index_stream_carry(const csv_fai_stream* s, int64_t* carry /* [3] */);
int csv_fasta_index_stream_rows(csv_fai_stream* s, const int64_t* rows, int64_t n_rows, const char* hdr, int64_t hdr_bytes, int64_t window_bytes,
                                const int64_t* tail /* [3] */);

/* The reference bases of the calls from somewhere else than chrom_seq (a BGZF-compressed FASTA: fasta.BgzfReference.gather).
 * csv_vcf_ref_ranges: per call c its contig chrom[c] (an index into chrom_name) and the bases [beg[c], end[c]) of it that the call's
 * record reads - INS [max(pos-1,0), +1), DEL [max(pos-1,0), min(pos+len, contig length)), DUP [pos, +1), INV the '++' / other rule,
 * BND either of its two indices; empty for a call the size filters drop, for INS / DEL under ignore_sequence, and for a BND call whose
 * base does not exist (its record says 'N').  chrom_len gives the contig lengths (0: the contig has no sequence); chrom_seq is not
 * read.  CSV_E_INVALID where csv_vcf_emit answers that: another call whose range is not inside its contig.
 * csv_vcf_emit_ref: csv_vcf_emit with the bases of call c's range taken from ref_blob[ref_off[c] .. ref_off[c + 1]) (n_calls + 1
 * offsets) in place of chrom_seq; CSV_E_INVALID also when a call's bytes are not as many as its range.  One function defines the
 * ranges for both and for csv_vcf_emit. */
int csv_vcf_ref_ranges(const csv_vcf_in* in, int64_t* beg, int64_t* end, int32_t* chrom);
int csv_vcf_emit_ref(const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, char* out, int64_t cap, int64_t* n_written, int64_t* svid);

/* The records on the device.  One rule writes a record for the host and for the device (csrc/vcf_core.h); these
 * entries give csv_vcf_emit_ref's text, byte for byte.
 * csv_vcf_emit_core_host: the rule with one lane and no context - csv_vcf_emit_ref's arguments and contract.
 * csv_vcf_emit_device: the same on the GPU.  `in` as it is (chrom_seq and the line arrays are not read); REF bases per call as
 *   csv_vcf_emit_ref takes them.  ALT and RNAMES come from the CSR blobs of `in` (uploaded), or - CSV_VCF_ALT_FROM_POOL, with pick / clip
 *   per INS call in call order as csv_seq_alt_gather takes them (int64); CSV_VCF_RNAMES_FROM_POOL, with the support lists of in->res -
 *   from the context's kept pool rebuild: csv_seq_alt_gather's and csv_name_support_join's kernels run, their blobs stay on the device,
 *   and their rules and refusals hold with the same texts.  prefix: bytes that stand in front of the records (a VCF header); out, rows'
 *   offsets and *n_written cover prefix + records.  rows (nullable): four int64 per emitted record, in emission order - {name index,
 *   beg, end, offset of the record} - the name index counting the chromosomes that emit a record in order of first appearance
 *   (name_chrom[k] <- the chromosome of name k, *n_names <- their number), beg / end the tabix interval of csv_tbx_build's rule.
 *   CSV_VCF_KEEP_TEXT: the text stays in the context (out may be NULL) until the next csv_vcf_emit_device; csv_vcf_text_fetch brings it
 *   down, csv_bgzf_deflate_text compresses it there, csv_vcf_text_info tells how many emits the context has seen and the kept bytes.
 *   CSV_OK; CSV_E_CAPACITY with the need in *n_written / *n_rows and nothing stored; CSV_E_INVALID with nothing stored wherever the host
 *   emitter says it, for what it would read outside its tables, and for a text of 2^31 - 4096 bytes or more.  Everything is judged on the
 *   host before a kernel is launched; svid advances only on success. */
enum { CSV_VCF_KEEP_TEXT = 1, CSV_VCF_ALT_FROM_POOL = 2, CSV_VCF_RNAMES_FROM_POOL = 4 };
int csv_vcf_emit_core_host(const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, char* out, int64_t cap, int64_t* n_written, int64_t* svid);
int csv_vcf_emit_device(csv_ctx* ctx, const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, int64_t n_pick, const int64_t* pick, const int64_t* clip,
                        const char* prefix, int64_t prefix_bytes, int32_t flags, char* out, int64_t cap, int64_t* n_written, int64_t* svid /* [5] */, int64_t* rows,
                        int64_t rows_cap, int64_t* n_rows, int32_t* name_chrom, int32_t* n_names, double* ms_kernels);
int csv_vcf_text_info(csv_ctx* ctx, int64_t* gen, int64_t* bytes);
int csv_vcf_text_fetch(csv_ctx* ctx, char* out, int64_t cap, int64_t* need);

/* ---------------------------------------------------------------------------------------------
 * Host-side row builder: the structure-of-arrays result -> the row lists the reference's resolvers return
 * (DEL 13 fields INDEL:207-219 / 464-478, INS 14 INDEL:419-432, DUP 11 DUP:121-131 / 170-180, INV 12 INV:145-156 /
 * 240-251, TRA 12 TRA:171-182), as ONE text blob: fields separated by '\t', rows terminated by '\n', rows in call
 * order (row c belongs to segment res->call_seg[c]).  All numeric fields are decimal text, read names joined by ','
 * exactly as the reference's rows hold them.  The Python shim splits the blob once (cutesv_amd/rows.py); any other
 * host language can do the same.  No GPU work: plain C++ on the caller's thread.
 */
typedef struct csv_rows_in {
    const csv_batch_out* res;
    const csv_segment*   seg;
    int32_t              n_seg;
    int32_t              n_chrom;
    const char* const*   chrom_name;     /* n_chrom */
    const int32_t*       read_id;        /* the batch's read_id column (support_sig indexes it) */
    const int32_t*       aux;            /* the batch's aux column (length of a synthetic inserted sequence) */
    /* read names: a table (blob + n_names + 1 offsets) or, when name_blob is NULL, "<name_prefix><id zero-padded to
     * name_width digits>" (the naming scheme of the synthetic workloads) */
    const char*          name_blob;
    const int64_t*       name_off;
    int64_t              n_names;
    const char*          name_prefix;
    int32_t              name_width;
    int32_t              n_strand;
    /* inserted sequences by global signature index (blob + n_sig + 1 offsets); NULL = "ACGT" repeated to aux[sig] */
    const char*          ins_blob;
    const int64_t*       ins_off;
    const char* const*   strand_name;    /* INV: call_aux -> strand text */
    /* cal_GL's strings per table row: CSV_GL_TABLE_SIZE entries "GT\tPL\tGQ\tQUAL" as blob + offsets */
    const char*          gl_blob;
    const int64_t*       gl_off;
} csv_rows_in;

/* Writes the rows into `out` (capacity `cap`) and returns CSV_OK, or CSV_E_CAPACITY with *n_written = the need. */
int csv_rows_emit(const csv_rows_in* in, char* out, int64_t cap, int64_t* n_written);

/* ---------------------------------------------------------------------------------------------
 * Native BAM reader: a coordinate-sorted .bam -> the columns the extraction entries take.
 *
 * Host side (no GPU, no context): csv_bam_open maps the file, indexes its BGZF blocks, reads the BAM header and refuses a
 * file whose blocks are truncated or whose end-of-file block is missing.  csv_bam_read inflates blocks on `threads` host
 * threads, walks the block_size chain and hands out one chunk: the records of reference `refid` (-1: the unmapped tail)
 * that overlap [beg, end) - pos < end and pos + max(reference span, 1) > beg - at most max_records of them.  Without an index
 * (csv_bam_index_load, below) the scan starts at the contig (or where the previous region of the same contig started) and stops at the
 * first record with pos >= end.  CSV_BAM_RESTART begins a new scan; without it the call continues behind the previous
 * chunk (more = 1 said there is one).  CSV_BAM_COUNT_ONLY counts records and packs nothing.
 *
 * A chunk is two byte images.  `slim` goes to the device: per record the 32 fixed bytes that follow block_size, the CIGAR
 * words and the aux bytes, rec_len[i] bytes at rec_off[i] (16-byte aligned, zero padded).  `host` stays behind: per
 * record the read name (l_read_name bytes, NUL included) and the 4-bit sequence, at host_off[i] .. host_off[i + 1].
 * Qualities are dropped.  The arrays belong to the reader and live until its next csv_bam_read / csv_bam_close.
 */
typedef struct csv_bam csv_bam;

typedef struct csv_bam_chunk {
    int64_t         n_records;
    int32_t         more;            /* 1: max_records was reached, the next call (without CSV_BAM_RESTART) continues */
    int32_t         reserved;
    const uint8_t*  slim;   int64_t slim_bytes;
    const int64_t*  rec_off;         /* n_records */
    const uint32_t* rec_len;         /* n_records */
    const uint8_t*  host;   int64_t host_bytes;
    const int64_t*  host_off;        /* n_records + 1 */
    int64_t         record_bytes;    /* inflated bytes of the chunk's records (block_size words included) */
    int64_t         inflated_bytes, compressed_bytes;    /* BGZF blocks inflated during the call */
    double          ms_inflate, ms_frame;                /* host wall time: inflate; framing + packing */
} csv_bam_chunk;
enum { CSV_BAM_RESTART = 1, CSV_BAM_COUNT_ONLY = 2 };

int         csv_bam_open(const char* path, int threads, csv_bam** out, char* err, int err_cap);
void        csv_bam_close(csv_bam* bam);
const char* csv_bam_error(const csv_bam* bam);
/* names: n_ref NUL-terminated strings back to back; text: the SAM header text (text_len bytes) */
int         csv_bam_header(const csv_bam* bam, int32_t* n_ref, const char** names, const int64_t** lengths, const char** text, int64_t* text_len);
int         csv_bam_read(csv_bam* bam, int32_t refid, int64_t beg, int64_t end, int64_t max_records, int32_t flags, csv_bam_chunk* out);
/* sizeof of 0 csv_bam_chunk, 1 csv_bam_in, 2 csv_bam_out; -1 otherwise */
int         csv_bam_struct_size(int which);

/* The BAM index (.bai; parsed by csrc/bai_index.h from the SAM specification, section 5.2).
 *
 * csv_bam_index_load reads and validates an index and keeps, per reference, its linear index (one virtual offset per 16 384-base
 * window) and the counts of the pseudo-bin 37450, and per file n_no_coor.  path == NULL: "<bam path>.bai" is tried, then the BAM
 * path with ".bam" replaced by ".bai".  CSV_E_STATE: no such file (the reader stays as it was).  CSV_E_INVALID, with a
 * csv_bam_error text that names the index file: no "BAI\1" magic; n_ref is not the BAM header's; a negative or absurd n_bin,
 * n_chunk or n_intv; the file ends inside a field; a linear-index entry below the one before it (zeros aside); a virtual offset
 * whose coffset is not the start of a BGZF block of THIS file or whose uoffset is above that block's ISIZE.  A reader whose load
 * failed has no index.  csv_bam_index_drop forgets the index.
 *
 * With an index loaded a scan of csv_bam_read / csv_bam_read_ranges with CSV_BAM_RESTART starts at the linear-index entry of the
 * window that holds `beg` (a zero entry means "no record": the next non-zero entry is taken; a window at or behind n_intv, or a
 * reference with n_bin == 0 and n_intv == 0, has no record: the call returns an empty chunk and touches no block), and blocks are
 * inflated ahead only up to where the index lets the region be expected to end.  The contract: THE INDEX ONLY MOVES THE
 * STARTING POINT.  The records of a region, their order and both images are byte for byte those of the forward scan;
 * compressed_bytes / inflated_bytes of a read that starts with no window inflated are never larger.  The unmapped tail (refid -1) is always found by the forward scan.
 *
 * csv_bam_index_stats: mapped[r] / unmapped[r] for every reference of the header (arrays of n_ref; either may be NULL) - zeros
 * for a reference without the pseudo-bin, as htslib reports - and *n_no_coor, -1 when the file does not carry it.  CSV_E_STATE
 * without an index.
 *
 * csv_bam_read_ranges: csv_bam_read for n_ranges >= 1 ranges [beg[i], end[i]) of one reference, sorted and disjoint (beg[i] <=
 * end[i] <= beg[i + 1]; CSV_E_INVALID otherwise).  One chunk sequence: every record that overlaps any range appears once, in file
 * order - the overlap rule, max_records, `more` (the next call without CSV_BAM_RESTART, with the same ranges, continues) and
 * CSV_BAM_COUNT_ONLY are csv_bam_read's.  With an index the cursor jumps to the entry of the next range's first window when that
 * lies ahead; inside a call it only moves forward.  Without one the ranges are served by one forward scan. */
int         csv_bam_index_load(csv_bam* bam, const char* path);
int         csv_bam_index_drop(csv_bam* bam);
int         csv_bam_index_stats(const csv_bam* bam, int64_t* mapped, int64_t* unmapped, int64_t* n_no_coor);
/* the number of the BGZF block (0 = the file's first) a read of `refid` from `beg` on starts in; -1: the index has no record there;
 * -2: no index, no reader, or a refid outside the header */
int64_t     csv_bam_index_block(const csv_bam* bam, int32_t refid, int64_t beg);
int         csv_bam_read_ranges(csv_bam* bam, int32_t refid, int32_t n_ranges, const int64_t* beg, const int64_t* end, int64_t max_records, int32_t flags,
                                csv_bam_chunk* out);

/* Building the index a file came without (csrc/index_core.h).  csv_bam_index_build (flags: 0) runs one pass over
 * the whole file on the reader's current routes - with csv_bam_set_frame the index kernels work on the rows of every framed window,
 * which stay in device memory; otherwise a host loop walks the records through the same core - and assembles the bytes of a .bai file:
 * bins with their chunks, the pseudo-bins 37450, the linear index with empty windows filled from the next one, n_no_coor; byte for byte
 * what tests/bai_writer.py, the test suite's independent reading of SAMv1 5.2 / 5.3 with htslib's conventions, writes.  The bytes are then parsed and validated as a file's
 * are (csv_bam_index_load) and installed: from then on the reader has an index.  *n_bytes (may be NULL): their number.
 * CSV_E_INVALID with a csv_bam_error text "cannot build the index: record <ordinal> ..." and nothing installed (an index the
 * reader had stays): a record that reaches 2^29 bases or beyond (the BAI format cannot index it); that ends beyond max(l_ref, 1) of
 * its reference; whose refID the header does not have; or that is out of coordinate order against the record before it (a lower
 * refID, -1 sorting last, or the same reference and a lower pos).  The texts are the same on every route.  A damaged block or a
 * broken record chain gives the reader's own error.  The build counts as a read: a device chunk handed out before it is dead.
 * csv_bam_index_bytes: the bytes of a BUILT index into out[0 .. cap); *need = their number.  CSV_E_STATE: the reader has no index,
 * or one loaded from a file (whose bins were not kept); CSV_E_CAPACITY: cap is too small, *need says what it takes, nothing is stored.
 * csv_bam_index_build_stats, of the last build: records indexed, runs (chunks before the join across windows), device time of all
 * kernels of the pass, bytes copied up and down by the framing route (0 on the host routes), csv_frame_run calls and index windows. */
int         csv_bam_index_build(csv_bam* bam, int32_t flags, int64_t* n_bytes);
int         csv_bam_index_bytes(const csv_bam* bam, uint8_t* out, int64_t cap, int64_t* need);
int         csv_bam_index_build_stats(const csv_bam* bam, int64_t* records, int64_t* runs, double* ms_kernels, int64_t* bytes_up, int64_t* bytes_down,
                                      int64_t* frame_runs, int64_t* index_windows);

/* The CSI index (.csi; parsed by csrc/csi_index.h, which restates the format): what `samtools index -c` writes,
 * and the only index a BAM with a contig of 2^29 bases or more can have.  csv_bam_index_load tells the format by content - a file
 * whose first member is a BGZF block with a payload that begins "CSI\1" is a CSI index, inflated with the reader's host BGZF code and
 * validated like a .bai (the magic; n_ref; negative or absurd counts; min_shift < 1, depth < 0 or min_shift + 3 * depth > 62; a bin
 * above the pseudo-bin; a pseudo-bin without two chunks; a chunk that ends before it begins; the end of the payload inside a field;
 * the virtual offsets; a loffset behind a chunk of its own bin or decreasing with the bin's first base).  With path == NULL,
 * "<bam path>.csi" and the BAM path with ".bam" replaced by ".csi" are tried after the two .bai names.  A region's scan starts at the
 * loffset of the bin with the greatest first base at or in front of `beg`, else at the reference's first record: coarser than a
 * .bai's linear index wherever the 2^min_shift-base bin at `beg` is not in the file, and under the same contract.  Everything above
 * (csv_bam_index_stats, csv_bam_index_block, csv_bam_read_ranges) works unchanged.  csv_bam_index_format says what the reader has.
 *
 * csv_bam_index_build_csi is csv_bam_index_build for a CSI index of 2^min_shift-base windows (4 .. 31; htslib's default is 14) and
 * `depth` levels under the root (0: htslib's rule, the smallest depth with max(l_ref) + 256 <= 2^(min_shift + 3 * depth)): the same
 * pass on the same routes, the same refusals with the range now 2^(min_shift + 3 * depth), in a text that names min_shift and depth.
 * On the framing route the linear arrays stay on the device: k_index_loff gathers one loffset per bin.  csv_bam_index_bytes then gives
 * the bytes of the .csi FILE (BGZF blocks and the end-of-file block), csv_bam_index_payload the payload they inflate to (CSV_E_STATE
 * unless the reader holds a built CSI index; CSV_E_CAPACITY as csv_bam_index_bytes).  csv_bam_index_build_stats_csi, of the last CSI
 * build: the bins written (the pseudo-bins aside) and the device time of k_index_loff (0 on the host routes). */
#define CSV_BAM_INDEX_NONE 0
#define CSV_BAM_INDEX_BAI  1
#define CSV_BAM_INDEX_CSI  2
int         csv_bam_index_format(const csv_bam* bam);
int         csv_bam_index_build_csi(csv_bam* bam, int32_t min_shift, int32_t depth, int64_t* n_bytes);
int         csv_bam_index_payload(const csv_bam* bam, uint8_t* out, int64_t cap, int64_t* need);
int         csv_bam_index_build_stats_csi(const csv_bam* bam, int64_t* bins, double* ms_loff);

/* Coordinate-sorting a BAM file (csrc/sort_core.h): what an aligner wrote -> the file this reader takes, with no
 * other tool.  csv_bam_sort runs one pass over the whole open file on the reader's current routes - the inflated bytes of every window
 * are appended to one arena in ctx's device memory (device to device when the reader frames there, uploaded otherwise), the record
 * starts come from the framed rows or from a host walk - and then, on ctx: k_sort_keys (key = refid' << 33 | (pos + 1) << 1 | reverse
 * bit with refid' = n_ref for refid -1; so a contig's pos -1 records come first, forward before reverse, records without a reference
 * last), the stable radix passes of the rebuild's permutation sort over the digits some key uses, the lengths' prefix sums, and per
 * slice of at most slice_blocks (0: 256; at most 32768) BGZF blocks of 65280 bytes k_sort_gather and the device compressor; only the
 * compressed blocks come down.  Records of equal key keep their input order.  The file written to out_path is the header with its
 * text changed in one place (@HD's SO: field becomes SO:coordinate, appended when absent; GO: and SS: fields are dropped; a text
 * without @HD gets "@HD\tVN:1.6\tSO:coordinate\n" in front; no @PG line is added), the records in order, and the end-of-file block.
 * csv_bam_sort_host is the core's host form: no context, the reader's host framing, std::stable_sort and csv_bgzf_deflate_host - the
 * same file byte for byte.  flags: 0 (none is defined).  out_path is created only after the verdict and removed when a later step
 * fails; the caller owns the rule for a file that exists (cutesv_amd.bam.sort_bam writes beside the target and renames).
 * CSV_E_CAPACITY, before the first window is read, with a csv_bam_error text that names both numbers: the inflated stream plus one
 * slice exceed max_bytes (<= 0: half of the device's free memory at the call; the host form: no limit).  Files beyond the budget are
 * not sorted here: no run files, no merge.  CSV_E_INVALID with the text "cannot sort: record <ordinal> ..." and nothing written: a refID
 * outside [-1, n_ref) or a pos below -1; the texts are the same on both forms.  CSV_E_NOMEM with a text: a table that cannot be
 * allocated.  A damaged block or a broken record chain gives the reader's own error.  The sort counts as a read: a device chunk
 * handed out before it is dead; an index the reader has stays.
 * csv_bam_sort_stats, of the last sort: counts[10] = records, inversions (adjacent pairs key[i] < key[i - 1] of the input: 0 means it
 * was in order), inflated bytes of the input, bytes of the sorted stream, bytes of the file, BGZF blocks (the end-of-file block
 * included), slices, radix passes run (0 on the host form), bytes copied up and down (0 on the host form); ms[4] = device time of the
 * key kernel, of the passes with the prefix sums, of the gather, of the compressor.  csv_bam_sort_blocks: the block table {uoff, coff,
 * isize} of the file, one row per block; *need = the rows; CSV_E_STATE: nothing was sorted; CSV_E_CAPACITY: cap is below *need. */
int csv_bam_sort(csv_bam* bam, csv_ctx* ctx, const char* out_path, int64_t max_bytes, int32_t slice_blocks, int32_t flags);
int csv_bam_sort_host(csv_bam* bam, const char* out_path, int64_t max_bytes, int32_t slice_blocks, int32_t flags);
int csv_bam_sort_stats(const csv_bam* bam, int64_t* counts, double* ms);
int csv_bam_sort_blocks(const csv_bam* bam, int64_t* uoff, int64_t* coff, uint32_t* isize, int64_t cap, int64_t* need);

/* SAM text -> BAM file (csrc/sam_core.h): what `minimap2 -a` writes -> the file csv_bam_sort takes, with no other
 * tool.  The leading @ lines become the header (text verbatim, references from the @SQ lines in order); every alignment line becomes
 * one record by the rules of SAMv1 1.4 / 4.2: names looked up in the @SQ names, POS and PNEXT minus one, bin = reg2bin(pos, pos +
 * max(reference length, 1)) & 0xffff, SEQ as 4-bit codes of =ACMGRSVTWYHKDBN without regard to case, QUAL minus 33 (`*`: 0xff), an `i`
 * tag in the smallest of c C s S i I, `f` as (float) strtod(text), a CIGAR of more than 65535 operations as the <l_seq>S<span>N
 * placeholder with a CG:B:I tag behind the line's own tags.  The stream is cut into BGZF blocks of 65280 bytes and the end-of-file
 * block is appended: the file is a pure function of the text, not of window_bytes (text per window; 0: 64 MiB; a longer line makes its
 * window grow) and not of the route.
 * csv_sam_to_bam: the device route.  The text goes up window by window; k_sam_marks, k_sam_plan, one scan, k_sam_small and k_sam_bulk
 * write the records into device memory, where the device compressor takes them; lines outside the device's strict grammar (every line
 * that may be refused; B:f arrays) are computed on the host one by one, floats outside the fast path of sam_core.h come back as four
 * bytes each.  flags: none is defined.  csv_sam_to_bam_host: the core's serial form over line ranges on `threads` host threads (0: 1)
 * and csv_bgzf_deflate_host; the same file byte for byte.  Both create the file only after the first window's verdict and remove it
 * when a later step fails.  CSV_E_INVALID with the text "line <1-based line of the file> <why>" (csv_last_error / err): the lowest
 * refused line; also a header without @SQ before alignment lines, an @SQ line without SN or LN, a reference named twice.
 * csv_sam_stats (ctx NULL: of this thread's last csv_sam_to_bam_host): counts[12] = lines, records, header bytes (the BAM header),
 * text bytes, stream bytes, file bytes, BGZF blocks (the end-of-file block included), windows, floats outside the fast path, CG
 * records, bytes up, bytes down; ms[4] = device time of the marks, the plan, the scan and write kernels, the compressor.
 * csv_sam_records: the line rule over text[0, n) (whole lines; the last may lack its line break) without files, on the host: the
 * records back to back in out[0, *need); the names are name_blob[name_off[i], name_off[i + 1]) in header order; first_line: the 1-based
 * number the first line is reported as; counts (may be NULL): lines, floats outside the fast path, CG records.  CSV_E_CAPACITY: cap is
 * below *need. */
int csv_sam_to_bam(csv_ctx* ctx, const char* sam_path, const char* out_path, int64_t window_bytes, int32_t flags);
int csv_sam_to_bam_host(const char* sam_path, const char* out_path, int64_t window_bytes, int32_t threads, char* err, int err_cap);
int csv_sam_stats(const csv_ctx* ctx, int64_t* counts, double* ms);
int csv_sam_records(const uint8_t* text, int64_t n, int32_t n_ref, const uint8_t* name_blob, const int32_t* name_off, int64_t first_line, uint8_t* out, int64_t cap,
                    int64_t* need, int64_t* counts, char* err, int err_cap);

/* BGZF inflate on the device: the raw-deflate payloads of n_blocks BGZF blocks -> their bytes, one wavefront
 * per block.  Block k's payload is comp[in_off[k] .. + in_len[k]), its out_len[k] (= ISIZE) bytes go to out[out_off[k] ..), crc[k]
 * is the CRC32 of its trailer; comp, out and status are host memory.
 *   status[k] == 0: out[out_off[k] .. + out_len[k]) holds exactly what zlib's inflate with Z_FINISH gives for the payload, and its
 *   CRC32 is crc[k].  Otherwise the byte says why (CSV_INF_E_*), the block's bytes are unspecified - but nothing outside its own
 *   range was written - and the caller inflates it again on the host if it wants a verdict it can report.  Bytes behind the final
 *   deflate block are ignored, as zlib ignores them.  A block with out_len == 0 is skipped with status 0.  Bytes of `out` that
 *   belong to no block are not written.
 * The return value is CSV_OK whenever the call was well-formed: damaged blocks are reported per block.  CSV_E_INVALID, nothing
 * launched: a payload outside comp, an output outside out, out_len above 65536, in_len < 0, overlapping outputs, n_blocks < 0,
 * flags != 0 (none is defined).  *ms_kernels (may be NULL): device time of the kernel.
 * The entry uses device buffers of its own and leaves everything else the context holds as it is: the columns of the last
 * csv_bam_decode and their gates, the pools, a kept rebuild.
 * The byte has eight bits for the nine reasons of a damaged block: a bad block type and a stored block whose LEN and NLEN
 * disagree share CSV_INF_E_HEADER. */
enum {
    CSV_INF_E_HEADER = 1,      /* block type 3; stored LEN / NLEN mismatch */
    CSV_INF_E_LENGTHS = 2,     /* over-subscribed or incomplete code lengths, too many of them, no end-of-block code */
    CSV_INF_E_SYMBOL = 4,      /* literal/length 286 / 287, distance 30 / 31, a repeat code with nothing before it, bits that are no code */
    CSV_INF_E_DISTANCE = 8,    /* a distance beyond the bytes produced so far in THIS block */
    CSV_INF_E_OUTPUT = 16,     /* the output would pass out_len */
    CSV_INF_E_SHORT = 32,      /* the stream ended (BFINAL done) short of out_len */
    CSV_INF_E_INPUT = 64,      /* input exhausted */
    CSV_INF_E_CRC = 128        /* CRC mismatch */
};
int csv_bgzf_inflate(csv_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len,
                     const int64_t* out_off, const int32_t* out_len, const uint32_t* crc, uint8_t* out, int64_t out_bytes, int32_t flags,
                     uint8_t* status, double* ms_kernels);
/* The reader's inflate route.  ctx != NULL: csv_bam_read inflates its windows with csv_bgzf_inflate on that context, window_blocks
 * BGZF blocks per call (<= 0: the default, CSV_BAM_WINDOW_BLOCKS; at most 16384), into a page-locked window out of which the records
 * are framed in place; every block the device reports with a non-zero status is inflated again on the host, whose verdict stands: a
 * damaged file gives the error text of the host route.  ctx == NULL: back to the host threads.  The context must outlive the reader
 * or be taken away before it is destroyed.  What a chunk contains does not depend on the route. */
#define CSV_BAM_WINDOW_BLOCKS 4096
int csv_bam_set_inflate(csv_bam* bam, csv_ctx* ctx, int32_t window_blocks);
/* since the start of the last csv_bam_read: blocks the device inflated, blocks the host inflated again, device time of the kernels */
int csv_bam_inflate_stats(const csv_bam* bam, int64_t* device_blocks, int64_t* fallback_blocks, double* ms_kernels);

/* BGZF deflate on the device: n_blocks pieces of at most 65280 bytes -> complete BGZF blocks, packed back to
 * back into a file image, one wavefront per block (deflate_core.h).  Block k's input is in[in_off[k] .. + in_len[k]); in, out and
 * block_bytes are host memory.  block_bytes[k]: the size of block k's BGZF block (header, raw-DEFLATE payload, CRC32, ISIZE; at most
 * in_len[k] + 31: per block the smallest of the stored, the fixed and the dynamic coding is written); *out_bytes: their sum.  When that
 * sum is at most out_cap the image is in out[0 .. *out_bytes); when it is larger the call still returns CSV_OK, *out_bytes tells the
 * need and no byte of `out` is written.  The bytes are a pure function of each input block: csv_bgzf_deflate_host, the core's host form,
 * gives the same bytes; they need not be zlib's, but zlib inflates them to the input.  No end-of-file block is appended.
 * CSV_E_INVALID, nothing launched: a null pointer, a negative count, in_len[k] > 65280, an input range outside `in`, flags != 0 (none
 * is defined).  *ms_kernels (may be NULL): device time of the kernels.  The entry uses device buffers of its own and leaves
 * everything else the context holds as it is. */
int csv_bgzf_deflate(csv_ctx* ctx, const uint8_t* in, int64_t in_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len,
                     uint8_t* out, int64_t out_cap, int32_t* block_bytes, int64_t* out_bytes, int32_t flags, double* ms_kernels);
/* the same on the host, one thread, no context.  coding_bytes (may be NULL): 3 per block - the payload bytes of the stored, the fixed
 * and the dynamic coding of the block's tokens, of which the smallest was written */
int csv_bgzf_deflate_host(const uint8_t* in, int64_t in_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len,
                          uint8_t* out, int64_t out_cap, int32_t* block_bytes, int64_t* out_bytes, int32_t* coding_bytes);
/* The tabix index of VCF text that was compressed in the BGZF blocks {uoff, coff, isize} (n_blocks >= 1 rows, the end-of-file block
 * included): the bytes of the .tbi BEFORE its own BGZF compression.  Lines that start with '#' are skipped; the names are the distinct
 * CHROM values in order of first appearance; a line's interval is [POS - 1, END) with END the value of INFO's END= key when that is
 * greater than POS - 1, else POS - 1 + len(REF); bins, 16 kb windows and virtual offsets as in the BAM index.  *out_bytes: the size;
 * nothing is written when it exceeds out_cap.  CSV_E_INVALID with a text in err: a line out of coordinate order, a contig that
 * reappears, a position at or beyond 2^29, a line without a numeric POS - named by the ordinal of the data line, from 0. */
int csv_tbx_build(const char* text, int64_t text_bytes, int64_t n_blocks, const int64_t* uoff, const int64_t* coff, const uint32_t* isize,
                  uint8_t* out, int64_t out_cap, int64_t* out_bytes, char* err, int32_t err_cap);
/* csv_bgzf_deflate with the context's kept VCF text (CSV_VCF_KEEP_TEXT) as its input; CSV_E_INVALID also when there is none or a range
 * lies outside it.  csv_tbx_build_rows: pass 2 of csv_tbx_build fed from csv_vcf_emit_device's rows instead of the text - names back to
 * back with n_names + 1 offsets, record r's bytes end where record r + 1 starts, the last at text_bytes - the same bytes, the same
 * refusals by ordinal. */
int csv_bgzf_deflate_text(csv_ctx* ctx, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, uint8_t* out, int64_t out_cap, int32_t* block_bytes,
                          int64_t* out_bytes, double* ms_kernels);
int csv_tbx_build_rows(const char* names, const int64_t* name_off, int32_t n_names, const int64_t* rows, int64_t n_rows, int64_t text_bytes, int64_t n_blocks,
                       const int64_t* uoff, const int64_t* coff, const uint32_t* isize, uint8_t* out, int64_t out_cap, int64_t* out_bytes, char* err, int32_t err_cap);

/* Reference bases out of a BGZF-compressed FASTA: n_ranges base ranges, cut out of the n_blocks BGZF blocks
 * they touch, on the device.  Block k: the raw-deflate payload comp[in_off[k] .. + in_len[k]), which inflates to the isize[k] (0 ..
 * 65536) bytes at the uncompressed offsets [uoff[k], uoff[k] + isize[k]) with CRC32 crc[k]; the blocks are sorted by uoff and do not
 * overlap; they need not be adjacent.  Range r: bases [beg[r], end[r]) of a contig whose first base sits at uncompressed offset
 * base_off[r], with line_bases[r] bases per line of line_width[r] bytes - base i lies at base_off + (i / lb) * lw + i % lb.  Ranges may
 * be unsorted, empty, equal or overlapping.  out receives the bases of the ranges in order, line breaks left out; out_off the n_ranges
 * + 1 offsets; *out_bytes their sum.  When that exceeds out_cap the call still returns CSV_OK, *out_bytes tells the need, and no byte
 * of `out` or of block_status is written.  block_status[k]: csv_bgzf_inflate's status byte of block k (all 0 when no range has a
 * base: nothing is inflated then); the bytes of ranges that read a block with a non-zero status are unspecified, and nothing outside
 * out[0, *out_bytes) is written.  CSV_E_INVALID with a text, nothing launched and nothing written: a null pointer, a negative count,
 * line_bases <= 0, line_width < line_bases, beg < 0, end < beg, overlapping or unsorted blocks, a payload outside comp, flags != 0
 * (none is defined), a range any of whose source bytes lies in none of the blocks (named by its ordinal).  ms_kernels (may be NULL):
 * device time of the inflate and of the gather.  The entry uses device buffers of its own and leaves everything else the context
 * holds as it is. */
int csv_ref_gather(csv_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len,
                   const int64_t* uoff, const int32_t* isize, const uint32_t* crc, int64_t n_ranges, const int64_t* base_off,
                   const int32_t* line_bases, const int32_t* line_width, const int64_t* beg, const int64_t* end, uint8_t* out, int64_t out_cap,
                   int64_t* out_off, int64_t* out_bytes, uint8_t* block_status, int32_t flags, double* ms_kernels /* [2] */);
/* the same on the host, one thread, no context, from blocks that are inflated already: block k's bytes are data[data_off[k] .. +
 * isize[k]).  The refusal's text goes to err (may be NULL). */
int csv_ref_gather_host(const uint8_t* data, int64_t data_bytes, int32_t n_blocks, const int64_t* data_off, const int64_t* uoff,
                        const int32_t* isize, int64_t n_ranges, const int64_t* base_off, const int32_t* line_bases, const int32_t* line_width,
                        const int64_t* beg, const int64_t* end, uint8_t* out, int64_t out_cap, int64_t* out_off, int64_t* out_bytes,
                        char* err, int32_t err_cap);

/* The .fai of a BGZF-compressed FASTA on the device: one window of its text - the n_blocks adjacent blocks
 * whose text starts at uncompressed offset `base`, given as csv_ref_gather takes them - is inflated on the device and reduced there to
 * event rows: one row of 3 int64 per line that a line break inside the window ends and that matters (the window's first, a header,
 * the line after a header, a line whose bytes or bases differ from the line before).  carry[3]: csv_fasta_index_stream_carry's.
 * rows / *n_rows, tail[3] and hdr / *hdr_bytes are what csv_fasta_index_stream_rows takes.  *n_rows > row_cap or *hdr_bytes > hdr_cap:
 * the call returns CSV_OK, reports the need and fills neither; *n_rows == -1: a block has a non-zero status (block_status as
 * csv_bgzf_inflate's).  Such a window is the host's: inflate it there and feed its bytes.  A window holds at most 2^30 bytes.
 * ms_kernels (may be NULL): device time of the inflate and of the event kernels.  Device buffers of the entry's own, as csv_ref_gather. */
int csv_fai_events(csv_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len,
                   const int32_t* isize, const uint32_t* crc, int64_t base, const int64_t* carry /* [3] */, int64_t* rows, int64_t row_cap,
                   int64_t* n_rows, int64_t* tail /* [3] */, char* hdr, int64_t hdr_cap, int64_t* hdr_bytes, uint8_t* block_status,
                   double* ms_kernels /* [2] */);
/* the same on the host from the window's inflated bytes, no context: the twin (rows beyond row_cap are counted, not written) */
int csv_fai_events_host(const uint8_t* data, int64_t n, int64_t base, const int64_t* carry /* [3] */, int64_t* rows, int64_t row_cap,
                        int64_t* n_rows, int64_t* tail /* [3] */, char* hdr, int64_t hdr_cap, int64_t* hdr_bytes);

/* Record framing on the device, opt-in.  ctx != NULL: it must be the context of the reader's device inflate
 * route (csv_bam_set_inflate with the same ctx before; CSV_E_STATE otherwise).  From then on the inflated window stays in device
 * memory: the records are found there (frame_core.h: one wavefront per BGZF block guesses a record start and chases the chain
 * through its block, one lane stitches the blocks from the cursor - a guess that is not the offset the true chain arrives at is never
 * used, that block is chased again serially), only a table of one 40-byte row per framed record comes down, the selection loop of
 * csv_bam_read runs over the rows - the same checks in the same order, the same error texts - and the slim and the host image of the
 * selected records are built in device memory.  ctx == NULL: back to host framing.  csv_bam_set_inflate also switches back.
 * ONE reader frames on a context at a time: the window, the chunk and the *_framed consumers are the context's.  A second reader is
 * refused with CSV_E_STATE until the first has switched back - which it must do before it is closed (csv_bam_close does not touch
 * the context).
 * On this route csv_bam_chunk has slim == NULL and host == NULL; the byte counts, rec_off, rec_len, host_off, the counters and the
 * timings are filled as on the host route, and the images are, byte for byte, what the host route builds.  The device chunk is
 * valid until the reader's next read or route change:
 *   csv_bam_chunk_lengths   l_read_name and l_seq per record of the last chunk (either route; arrays of n_records, may be NULL)
 *   csv_bam_chunk_fetch     downloads the two images (slim_bytes / host_bytes bytes; either may be NULL) - for checks and for the
 *                           rare host fallbacks.  CSV_E_STATE: no device chunk of this reader is valid
 *   csv_bam_frame_stats     since the start of the last read: blocks whose guess was the true chain's, blocks chased again (fallbacks),
 *                           device time of the framing and pack kernels, bytes copied down and up by the framing route
 *   csv_bam_decode_framed, csv_name_pool_append_framed, csv_seq_reads_framed   csv_bam_decode (flags 0), csv_name_pool_append (the
 *                           names without their NUL) and csv_seq_reads_upload (`want` may be NULL) on the context's current device
 *                           chunk: they behave as their host-pointer twins do on the fetched images, and no image visits the host
 *                           (the decode copies the slim image device to device to where csv_bam_split_inputs and the gates expect it).
 *                           CSV_E_STATE: the context holds no valid device chunk */
int csv_bam_set_frame(csv_bam* bam, csv_ctx* ctx);
int csv_bam_chunk_lengths(const csv_bam* bam, int32_t* l_read_name, int32_t* l_seq);
int csv_bam_chunk_fetch(csv_bam* bam, uint8_t* slim, uint8_t* host);
int csv_bam_frame_stats(const csv_bam* bam, int64_t* right_blocks, int64_t* fallback_blocks, double* ms_kernels, int64_t* bytes_down, int64_t* bytes_up);
int csv_name_pool_append_framed(csv_ctx* ctx, int64_t* first_index);
int csv_seq_reads_framed(csv_ctx* ctx, const uint8_t* want);

/* Device side (bam.hip.h): the slim image of a chunk -> per-record columns, the packed CIGARs and the byte ranges of the
 * SA / CG tags, in device memory of the context (valid until its next csv_bam_decode; csv_cigar_signatures with
 * CSV_CG_FROM_BAM scans them in place, csv_bam_split_inputs parses the SA values there) and, for every host array that is not NULL, in the caller's memory.
 *   ref_start = pos, query_len = l_seq, ref_end = pos + lengths of M D N = X, clip_left / clip_right = length of the
 *   first / last CIGAR operation when it is S or H (else 0), cls = 0 secondary (flag 256 / 272), 1 primary (flag 0 / 16),
 *   2 other.  A record whose CIGAR is the placeholder <l_seq>S<n>N and that carries a CG:B,I tag (more than 65 535
 *   operations) is decoded from the tag.  sa_beg / sa_end: byte ranges, in `slim`, of the values of the record's SA:Z
 *   tags (sa_off[i] .. sa_off[i + 1], in tag order, NUL excluded); cg_beg / cg_end: of the CG array's words, -1 if none.
 * The aux walk knows the types A c C s S i I f Z H and B (subtypes c C s S i I f).  Any other type byte, or a value that
 * runs past the record, sets status[i] != 0, and the call fails with CSV_E_INVALID after the host arrays are filled.
 * CSV_E_CAPACITY: cap_ops / cap_sa are too small, n_ops / n_sa hold the need.
 */
typedef struct csv_bam_in {
    int64_t         n_records;
    const uint8_t*  slim;   int64_t slim_bytes;
    const int64_t*  rec_off;
    const uint32_t* rec_len;
    int32_t         flags;           /* 0 */
    int32_t         reserved;
} csv_bam_in;

typedef struct csv_bam_out {
    int64_t  cap_ops, cap_sa;        /* capacities of the host arrays cigar / sa_beg, sa_end */
    int64_t  n_ops, n_sa;            /* out */
    /* host arrays, each may be NULL: n_records entries (cig_off, sa_off: n_records + 1) */
    int64_t* ref_start;  int64_t* ref_end;  int32_t* flag;  int32_t* mapq;  int32_t* query_len;
    int32_t* clip_left;  int32_t* clip_right;  uint8_t* cls;  uint8_t* status;
    int64_t* cig_off;  uint32_t* cigar;
    int64_t* sa_off;  int64_t* sa_beg;  int64_t* sa_end;
    int64_t* cg_beg;  int64_t* cg_end;
    /* out: the same columns in device memory */
    void* dev_ref_start;  void* dev_ref_end;  void* dev_flag;  void* dev_mapq;  void* dev_query_len;
    void* dev_clip_left;  void* dev_clip_right;  void* dev_cls;  void* dev_cig_off;  void* dev_cigar;
    int64_t  bytes_uploaded;         /* out: slim image + offsets */
    int64_t  n_bad;                  /* out: records with status != 0 */
    float    ms_device;              /* out: kernels only (HIP events) */
    float    ms_upload;              /* out: host -> device copies (HIP events) */
} csv_bam_out;

int csv_bam_decode(csv_ctx* ctx, const csv_bam_in* in, csv_bam_out* out);
/* csv_bam_decode on the context's current device chunk (csv_bam_set_frame, above) */
int csv_bam_decode_framed(csv_ctx* ctx, csv_bam_out* out);

/* The SA tags of the context's last csv_bam_decode -> the entry columns of csv_split_in, parsed on the device (sa.hip.h,
 * DESIGN.md section 14).  A CALL is one (record i with sel[i] != 0, SA tag of that record) pair, in record order and then
 * tag order.  Its entries are the primary alignment when mapq[i] >= min_mapq (parse_read :660-668, from the decode's
 * columns: flag 0 -> c0 = clip_left, c1 = query_len - clip_right, strand 0; else the clips swapped, strand 1; f0 / f1 =
 * ref_start / ref_end, chr = task_rank, mapq 0, primary 1) and then one per "name,pos,strand,CIGAR,mapq[,...];" of the
 * value, in order (text behind the last ';' is dropped, as value.split(";")[:-1] drops it): chr = the rank of `name`,
 * f0 = pos - 1, strand 0 for '+' else 1, c0 / c1 / f1 = leading S length / trailing S length / span over M D = X of the
 * CIGAR text, mapq.  read_len = the record's query_len, call_rec = the record's index in the chunk.
 *
 * Contig names: n_names names back to back in `names` in ascending byte order, name k = bytes [name_off[k],
 * name_off[k + 1]), name_rank[k] = the caller's rank for it (any integers).
 *
 * The device accepts a strict grammar only: a name of the table; pos an unsigned decimal number of 1 - 18 digits, mapq
 * of 1 - 9; a strand of one character; a CIGAR that is "*" or a run of <1 - 18 digits><one of MIDNSHP=XB>; at least
 * five fields.  A call with any other entry gets status != 0 (bits: 1 number, 2 strand, 4 CIGAR, 8 fewer than five
 * fields, 16 unknown name), is counted in n_flagged and has NO entries: it is the caller's to parse (the Python layer
 * sends exactly those through encode_split_reads, so the reference's behaviour on such text, exceptions included, stays).
 *
 * The columns stay in device memory of the context until its next csv_bam_decode / csv_bam_split_inputs
 * (csv_split_signatures with CSV_SP_FROM_BAM reads them there); every host array that is not NULL is filled as well.
 * CSV_E_CAPACITY: a per-call array is given and cap_calls < n_calls, or a per-entry array and cap_entries < n_entries;
 * the counts hold the need.  CSV_E_INVALID, before anything is launched: no decode in the context, n_records is not the
 * decode's, or the name table is inconsistent (offsets that decrease or leave `names`, names not strictly ascending). */
typedef struct csv_sa_in {
    int64_t         n_records;
    const uint8_t*  sel;             /* n_records */
    int32_t         min_mapq;
    int32_t         task_rank;       /* rank of the contig the chunk lies on */
    int32_t         n_names;
    int32_t         flags;           /* 0 or CSV_SA_SEL_FROM_GATES */
    const uint8_t*  names;   int64_t name_bytes;
    const int64_t*  name_off;        /* n_names + 1 */
    const int32_t*  name_rank;       /* n_names */
} csv_sa_in;

typedef struct csv_sa_out {
    int64_t  cap_calls, cap_entries;
    int64_t  n_calls, n_entries, n_flagged;                 /* out */
    int64_t* ent_off;  int64_t* read_len;  int32_t* call_rec;  uint8_t* status;      /* cap_calls (ent_off: + 1) */
    int64_t* c0;  int64_t* c1;  int64_t* f0;  int64_t* f1;  int32_t* chr;  int32_t* mapq;  uint8_t* strand;  uint8_t* primary;   /* cap_entries */
    float    ms_device;              /* out: kernels only (HIP events) */
    int32_t  reserved;
} csv_sa_out;

/* csv_sa_in.flags: sel must be NULL, sel[i] is bit CSV_GATE_SEL of the gates csv_bam_task_gates left beside the decode.  CSV_E_INVALID,
 * nothing launched: `sel` is given as well, or the context holds no gates of its last csv_bam_decode. */
enum { CSV_SA_SEL_FROM_GATES = 1 };

int csv_bam_split_inputs(csv_ctx* ctx, const csv_sa_in* in, csv_sa_out* out);
/* sizeof of 0 csv_sa_in, 1 csv_sa_out; -1 otherwise */
int csv_sa_struct_size(int which);

/* The gates of an extraction task on the records of the context's last csv_bam_decode (gates.hip.h): one
 * byte of CSV_GATE_* bits per record, as single_pipe (cuteSV main script :711, :715-725) and parse_read (:607, :614) apply them.
 *   TASK    cls != 0 && ref_start >= task_start && in_bed        (in_bed is true without CSV_GT_BED)
 *   PARSED  TASK && query_len >= min_read_len
 *   USE     PARSED && mapq >= min_mapq                           (the `use` column of csv_cigar_signatures)
 *   SEL     PARSED && cls == 1 && the record has an SA tag       (the `sel` column of csv_bam_split_inputs)
 *   READS   TASK && mapq >= min_mapq                             (the rows of the reads table, :729-733)
 * CSV_GT_BED: in_bed = some region k has region_end[k] > ref_start && region_beg[k] < ref_end - the reference's
 * `not (pos_end <= b0 or pos_start >= b1)` on the list of the record's TASK (load_bed, cuteSV_genotype.py:704-726), applied as
 * written: a zero-span record (ref_end == ref_start) lies in no region it merely touches, regions are not merged, a region with
 * end < beg is legal.  region_beg must not decrease (load_bed sorts by (start, end)); 0 regions: no record passes.
 * The column stays in device memory of the context until its next csv_bam_decode - CSV_CG_USE_FROM_GATES and CSV_SA_SEL_FROM_GATES
 * read it there - and is copied to `bits` when that is not NULL; a later call on the same decode replaces it.  ms_device
 * (nullable): the kernel alone (HIP events).  n_records == 0 succeeds and launches nothing.
 * CSV_E_INVALID, before anything is launched, the context (and gates it already holds) unchanged: no decode in the context,
 * n_records is not the decode's, n_regions < 0, regions without CSV_GT_BED, CSV_GT_BED with n_regions > 0 and a NULL array,
 * region_beg that decreases, unknown flag bits. */
enum { CSV_GT_BED = 1 };
enum { CSV_GATE_TASK = 1, CSV_GATE_PARSED = 2, CSV_GATE_USE = 4, CSV_GATE_SEL = 8, CSV_GATE_READS = 16 };
int csv_bam_task_gates(csv_ctx* ctx, int64_t n_records, int64_t task_start, int32_t min_read_len, int32_t min_mapq, int32_t flags,
                       int64_t n_regions, const int64_t* region_beg, const int64_t* region_end,
                       uint8_t* bits /* n_records, nullable */, float* ms_device /* nullable */);

/* The genotyping reads table in device memory (reads.hip.h).  The reference's reads table (cuteSV main
 * script :729-733) has one row per record that passed the gates of its task with mapq >= min_mapq; every column of it exists on
 * the device once the task's chunk is decoded, so the table is cut out of them there and handed to the engine where it lies:
 *   start    ref_start (int32: BAM positions are int32 fields)        end      ref_end, saturating at INT32_MAX
 *   primary  cls == 1 (flag 0 or 16)                                  id       the name pool's index of the record's name
 * (13 bytes per row in device memory), grouped by chromosome in append order.  It belongs to the context and lives until
 * csv_reads_reset / csv_ctx_destroy.
 *
 * csv_reads_reset: empties the table and fixes the number of chromosomes.  csv_reads_rows: its row count.
 * csv_reads_append_decoded: the records of the context's last csv_bam_decode that belong in the table, in record order -
 *   keep == NULL: those whose byte in the gates column of THAT decode has CSV_GATE_READS (csv_bam_task_gates must have run on it);
 *   keep != NULL: n_records host bytes, non-zero = keep (the host-gated path).
 *   row = { ref_start, ref_end, cls == 1, name_base + record index }.  Flags, scan, compaction and conversion run on the device;
 *   nothing but the count comes back (n_appended, nullable).  n_records == 0 launches nothing; when no record is kept nothing is
 *   launched after the count.
 * csv_reads_append: rows from host arrays (0 <= start <= end, id >= 0).
 * Ordering contract of both: chrom must be at least the chromosome of the last row.  Inside a chromosome the rows may come in any
 *   order (csv_batch_in's reads table: "rows in ANY order inside a block").  After a failed append the table is unchanged.
 * csv_reads_get: rows [first, first + n) back to the host (any array may be NULL).
 * csv_reads_batch_columns: the table as csv_batch_in wants it with CSV_IN_READS_DEVICE | CSV_IN_READS_I32: reads_off[n_chrom + 1]
 *   to the host, the DEVICE addresses of the four columns into `out` (NULL for an empty table).  CSV_RD_RANK_FROM_NAMES: r_id[i] =
 *   rank[id[i]], the ranks of the context's name pool (csv_name_ranks' device column, computed first when an append made it stale,
 *   as CSV_RB_RANK_FROM_NAMES does), written to a column of its own: the table is not changed and the call can be repeated.  The
 *   addresses are valid until the next append, reset or csv_reads_batch_columns; csv_batch_upload / csv_cluster_batch copy the
 *   columns, so the table may change once they have returned.
 * csv_reads_timing: the kernels of the last append / the rank gather of the last csv_reads_batch_columns in milliseconds (HIP events).
 * CSV_E_INVALID, before anything is launched, the context and the table unchanged: a NULL context; no csv_reads_reset yet; chrom
 *   outside [0, n_chrom) or below the chromosome of the last row; no successful decode, or n_records that is not the decode's;
 *   keep == NULL while the context holds no gates of its current decode; name_base < 0 or name_base + n_records beyond INT32_MAX;
 *   a host row with start < 0, end < start or id < 0; csv_reads_get outside the table; csv_reads_batch_columns with an n_chrom that is
 *   not the table's or with unknown flag bits; CSV_RD_RANK_FROM_NAMES with an id at or beyond the name pool's row count. */
enum { CSV_RD_RANK_FROM_NAMES = 1 };
typedef struct csv_reads_dev {
    int64_t        n_reads;
    const int32_t* r_start;         /* DEVICE addresses: n_reads entries each */
    const int32_t* r_end;
    const uint8_t* r_primary;
    const int32_t* r_id;
} csv_reads_dev;
int csv_reads_reset(csv_ctx* ctx, int32_t n_chrom);
int csv_reads_rows(const csv_ctx* ctx, int64_t* n);
int csv_reads_append_decoded(csv_ctx* ctx, int32_t chrom, int64_t n_records, const uint8_t* keep /* nullable */, int64_t name_base, int64_t* n_appended);
int csv_reads_append(csv_ctx* ctx, int32_t chrom, int64_t n, const int32_t* start, const int32_t* end, const uint8_t* primary, const int32_t* id);
int csv_reads_get(csv_ctx* ctx, int64_t first, int64_t n, int32_t* start, int32_t* end, uint8_t* primary, int32_t* id);
int csv_reads_batch_columns(csv_ctx* ctx, int32_t flags, int32_t n_chrom, int64_t* reads_off /* n_chrom + 1 */, csv_reads_dev* out);
int csv_reads_timing(const csv_ctx* ctx, float* ms_append, float* ms_columns);
/* sizeof of 0 csv_reads_dev; -1 otherwise */
int csv_reads_struct_size(int which);

#ifdef __cplusplus
}
#endif
#endif /* CUTESV_HIP_H */
