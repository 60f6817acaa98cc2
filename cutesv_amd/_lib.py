"""Loader of libcutesv_hip.so (the HIP kernels + C ABI).  There is no CPU fallback: if the
extension is missing or does not load, importing this module's `lib()` raises."""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# CUTESV_AMD_LIB: load another build of the same library (A/B timing of kernel variants); never a CPU fallback
LIB_PATH = os.environ.get("CUTESV_AMD_LIB") or os.path.join(_HERE, "libcutesv_hip.so")
_LIB = None

# every symbol include/cutesv_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("csv_abi_version", C.c_int, []),
    ("csv_struct_size", C.c_int, [C.c_int]),
    ("csv_measure_copy_bandwidth", C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_double)]),
    ("csv_cache_flush", C.c_int, [C.c_void_p, C.c_int64]),
    ("csv_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("csv_device_info", C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    ("csv_ctx_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("csv_ctx_destroy", None, [C.c_void_p]),
    ("csv_last_error", C.c_char_p, [C.c_void_p]),
    ("csv_stage_name", C.c_char_p, [C.c_int]),
    ("csv_cluster_batch", C.c_int, [C.c_void_p, C.POINTER(_abi.BatchIn), C.POINTER(_abi.BatchOut)]),
    ("csv_batch_upload", C.c_int, [C.c_void_p, C.POINTER(_abi.BatchIn)]),
    ("csv_batch_run", C.c_int, [C.c_void_p, C.POINTER(_abi.RunStats)]),
    ("csv_batch_download", C.c_int, [C.c_void_p, C.POINTER(_abi.BatchOut)]),
    ("csv_ctx_sync", C.c_int, [C.c_void_p]),
    ("csv_batch_publish_async", C.c_int, [C.c_void_p, C.POINTER(_abi.BatchOut)]),
    ("csv_batch_publish_wait", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(_abi.BatchOut))]),
    ("csv_batch_reads_mode", C.c_int, [C.c_void_p]),
    ("csv_batch_validate", C.c_int, [C.c_void_p]),
    ("csv_batch_info", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    ("csv_batch_option", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("csv_gl_index", C.c_int32, [C.c_int64, C.c_int64]),
    ("csv_host_alloc", C.c_int, [C.c_int64, C.POINTER(C.c_void_p)]),
    ("csv_host_free", None, [C.c_void_p]),
    ("csv_host_register", C.c_int, [C.c_void_p, C.c_int64]),
    ("csv_host_unregister", C.c_int, [C.c_void_p]),
    ("csv_rows_emit", C.c_int, [C.POINTER(_abi.RowsIn), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_cigar_signatures", C.c_int, [C.c_void_p, C.POINTER(_abi.CigarIn), C.POINTER(_abi.CigarOut)]),
    ("csv_split_signatures", C.c_int, [C.c_void_p, C.POINTER(_abi.SplitIn), C.POINTER(_abi.SplitOut)]),
    ("csv_rebuild_signatures", C.c_int, [C.c_void_p, C.POINTER(_abi.RebuildIn), C.POINTER(_abi.RebuildOut)]),
    ("csv_rebuild_route", C.c_int, [C.c_void_p]),
    ("csv_pool_reset", C.c_int, [C.c_void_p]),
    ("csv_pool_rows", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_pool_append", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_name_pool_reset", C.c_int, [C.c_void_p]),
    ("csv_name_pool_rows", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_name_pool_append", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_name_ranks", C.c_int, [C.c_void_p, C.POINTER(_abi.NameRankOut)]),
    ("csv_name_pool_get", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("csv_name_struct_size", C.c_size_t, [C.c_int]),
    ("csv_seq_reads_upload", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_seq_option", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("csv_seq_query_reverse", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    ("csv_seq_pool_rows", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("csv_seq_pool_put", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_seq_pool_get", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("csv_seq_pool_half", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("csv_seq_info_get", C.c_int, [C.c_void_p, C.POINTER(_abi.SeqInfo)]),
    ("csv_seq_struct_size", C.c_int, [C.c_int]),
    ("csv_seq_alt_gather", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    ("csv_name_support_join", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("csv_pool_sigs_text", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_float)]),
    ("csv_aln_reset", C.c_int, [C.c_void_p, C.c_int32]),
    ("csv_aln_rows", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_aln_append_decoded", C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_aln_append", C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_aln_get", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_aln_layout", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("csv_aln_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("csv_aln_tra_genotype", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    ("csv_reads_reset", C.c_int, [C.c_void_p, C.c_int32]),
    ("csv_reads_rows", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_reads_append_decoded", C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_reads_append", C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_reads_get", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_reads_batch_columns", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(_abi.ReadsDev)]),
    ("csv_reads_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("csv_reads_struct_size", C.c_int, [C.c_int]),
    ("csv_bam_task_gates", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_float)]),
    ("csv_vcf_emit", C.c_int, [C.POINTER(_abi.VcfIn), C.c_char_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    ("csv_bam_open", C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]),
    ("csv_bam_close", None, [C.c_void_p]),
    ("csv_bam_error", C.c_char_p, [C.c_void_p]),
    ("csv_bam_header", C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ("csv_bam_read", C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(_abi.ChunkC)]),
    ("csv_bam_struct_size", C.c_int, [C.c_int]),
    ("csv_bam_index_load", C.c_int, [C.c_void_p, C.c_char_p]),
    ("csv_bam_index_drop", C.c_int, [C.c_void_p]),
    ("csv_bam_index_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_bam_index_block", C.c_int64, [C.c_void_p, C.c_int32, C.c_int64]),
    ("csv_bam_read_ranges", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(_abi.ChunkC)]),
    ("csv_bam_index_build", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    ("csv_bam_index_bytes", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_bam_index_build_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("csv_bam_index_format", C.c_int, [C.c_void_p]),
    ("csv_bam_index_build_csi", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("csv_bam_index_payload", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_bam_index_build_stats_csi", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ("csv_bam_sort", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_int32, C.c_int32]),
    ("csv_bam_sort_host", C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.c_int32, C.c_int32]),
    ("csv_bam_sort_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_bam_sort_blocks", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_sam_to_bam", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int64, C.c_int32]),
    ("csv_sam_to_bam_host", C.c_int, [C.c_char_p, C.c_char_p, C.c_int64, C.c_int32, C.c_char_p, C.c_int]),
    ("csv_sam_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_sam_records", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_char_p,
                                  C.c_int]),
    ("csv_bgzf_inflate", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                   C.c_void_p, C.POINTER(C.c_double)]),
    ("csv_bgzf_deflate", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_int32,
                                   C.POINTER(C.c_double)]),
    ("csv_bgzf_deflate_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    ("csv_tbx_build", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_char_p, C.c_int32]),
    ("csv_bam_set_inflate", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    ("csv_bam_inflate_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ("csv_bam_decode", C.c_int, [C.c_void_p, C.POINTER(_abi.BamIn), C.POINTER(_abi.BamOut)]),
    ("csv_bam_set_frame", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csv_bam_chunk_lengths", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_bam_chunk_fetch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_bam_frame_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("csv_bam_decode_framed", C.c_int, [C.c_void_p, C.POINTER(_abi.BamOut)]),
    ("csv_name_pool_append_framed", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("csv_seq_reads_framed", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csv_bam_split_inputs", C.c_int, [C.c_void_p, C.POINTER(_abi.SaIn), C.POINTER(_abi.SaOut)]),
    ("csv_sa_struct_size", C.c_int, [C.c_int]),
    ("csv_fasta_index", C.c_int64, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_fasta_index_stream_open", C.c_void_p, []),
    ("csv_fasta_index_stream_feed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("csv_fasta_index_stream_finish", C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    ("csv_fasta_index_stream_close", None, [C.c_void_p]),
    ("csv_fasta_index_stream_carry", C.c_int, [C.c_void_p, C.c_void_p]),
    ("csv_fasta_index_stream_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    ("csv_vcf_ref_ranges", C.c_int, [C.POINTER(_abi.VcfIn), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("csv_vcf_emit_ref", C.c_int, [C.POINTER(_abi.VcfIn), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    ("csv_vcf_emit_core_host", C.c_int, [C.POINTER(_abi.VcfIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    ("csv_vcf_emit_device", C.c_int, [C.c_void_p, C.POINTER(_abi.VcfIn), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_double)]),
    ("csv_vcf_text_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("csv_vcf_text_fetch", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("csv_bgzf_deflate_text", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ("csv_tbx_build_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64), C.c_char_p, C.c_int32]),
    ("csv_ref_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int32, C.c_void_p]),
    ("csv_ref_gather_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_char_p, C.c_int32]),
    ("csv_fai_events", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]),
    ("csv_fai_events_host", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64,
                                      C.POINTER(C.c_int64)]),
]


class ExtensionMissing(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ExtensionMissing(
                "%s not found: build it with `make -C cutesv_amd/csrc` (or __graft_entry__.build()). "
                "cutesv_amd has no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)          # AttributeError here == ABI mismatch, fail loudly
            fn.restype, fn.argtypes = res, args
        if L.csv_abi_version() != _abi.ABI_VERSION:
            raise ExtensionMissing("libcutesv_hip.so ABI %d != python side %d" % (L.csv_abi_version(), _abi.ABI_VERSION))
        # a stale build with the same ABI number: every struct must have the size of its mirror
        for size_of, table in ((L.csv_struct_size, _abi.STRUCT_SIZES), (L.csv_bam_struct_size, _abi.BAM_STRUCT_SIZES), (L.csv_sa_struct_size, _abi.SA_STRUCT_SIZES),
                               (L.csv_name_struct_size, _abi.NAME_STRUCT_SIZES), (L.csv_seq_struct_size, _abi.SEQ_STRUCT_SIZES),
                               (L.csv_reads_struct_size, _abi.READS_STRUCT_SIZES)):
            for i, (name, size) in enumerate(table):
                if size_of(i) != size:
                    raise ExtensionMissing("%s: sizeof(%s) is %d, its python mirror has %d bytes: rebuild the library" % (LIB_PATH, name, size_of(i), size))
        _LIB = L
    return _LIB
