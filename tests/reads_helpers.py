"""Helpers of tests/test_reads_table.py: decoded chunks of crafted records, keep masks, the reads table as call_bam built it
inline before reads.table_host existed, a synthetic batch with an awkward reads table, and device memory read back."""
import ctypes as C

import numpy as np

from cutesv_amd import _abi, bam, rebuild, synth
from cutesv_amd._lib import lib
from cutesv_amd.columns import Params

import bam_writer
import bed_helpers as bh

# 1 .. 1100: below, at and above a wavefront and a workgroup, more than one workgroup; 1023 .. 1025: the scan's tile of 1024 records
CHUNK_SIZES = (1, 63, 64, 65, 255, 256, 257, 1100, 1023, 1024, 1025)


def decode_chunk(ctx, tmp_path, n, seed=11):
    """n crafted + random records (bed_helpers.gate_records: secondary, supplementary, MAPQ 0 and zero-span ones among them) written,
    read back and decoded on the context -> (chunk, decoded columns)"""
    path = str(tmp_path / ("reads%d_%d.bam" % (n, seed)))
    bam_writer.write_bam(path, bh.GATE_REFS, bh.gate_records(n, seed))
    with bam.BamFile(path) as bf:
        chunk = bf.records("7", 0, 1 << 40)
    assert chunk.n == n
    return chunk, bam.decode(ctx, chunk, host_outputs=False)


def keep_masks(n):
    i = np.arange(n)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0] = 1; last[-1] = 7                            # (any non-zero byte keeps)
    return [("none", np.zeros(n, np.uint8)), ("all", np.ones(n, np.uint8)), ("alternating", (i % 2).astype(np.uint8)), ("first", first), ("last", last),
            ("last_lane", (i % 64 == 63).astype(np.uint8))]


def inline_table(tables, ranks, n_chrom):
    """the reads table exactly as call_bam assembled it before reads.table_host: the concatenation of the tasks' columns with the
    ids ranks[name_base + reads_index], through rebuild._reads_by_chrom"""
    rd = dict(chrom=np.concatenate([np.full(len(r["reads_index"]), ci, np.int64) for ci, r in tables]),
              start=np.concatenate([r["reads_start"] for _, r in tables]), end=np.concatenate([r["reads_end"] for _, r in tables]),
              primary=np.concatenate([r["reads_primary"] for _, r in tables]),
              read_id=ranks[np.concatenate([r["name_base"] + r["reads_index"] for _, r in tables])])
    return rebuild._reads_by_chrom(rd, n_chrom)


def hand_made_tasks():
    """three tasks as task_to_pool returns them with reads="host": chromosomes 0 and 2 (1 stays empty), one task without rows; the
    rows of chromosome 0 come from two tasks and are not in start order -> ([(chromosome, task dict)], ranks of 40 names)"""
    def task(name_base, index, start, span, cls):
        index = np.asarray(index, np.int64)
        return dict(name_base=name_base, reads_index=index, reads_start=np.asarray(start, np.int64), reads_end=np.asarray(start, np.int64) + np.asarray(span, np.int64),
                    reads_primary=(np.asarray(cls) == 1).astype(np.uint8))
    tasks = [(2, task(0, [0, 3, 4], [500, 100, 100], [50, 0, 900], [1, 2, 1])), (0, task(10, [], [], [], [])),
             (0, task(10, [1, 2, 9], [7000, 6500, 8000], [10, 20, 30], [1, 1, 2])), (0, task(25, [0, 14], [20, 9000], [5000, 1], [2, 1]))]
    ranks = np.random.default_rng(3).permutation(40).astype(np.int32)
    return tasks, ranks


def device_to_host(address, count, dtype):
    """`count` items of `dtype` at a device address, copied with the HIP runtime the library is linked with"""
    out = np.empty(count, dtype)
    if count == 0:
        return out
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "the HIP runtime library was not found"
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, address, out.nbytes, 2) == 0                 # hipMemcpyDeviceToHost
    return out


def synthetic_batch(seed=2027):
    """A three-contig batch with INS, DEL, DUP, INV and TRA segments, all genotyped (TRA from the reads table), whose reads table
    has a block in shuffled order (contig 0), an empty block (contig 1) and a block of one read (contig 2) ->
    (segments, a, b, read_id, aux, contig_len, reads dict with int32 start / end)"""
    st = synth.small_mixed(seed=seed, n_sites=24)
    p = Params.ont(genotype=True, genotype_tra=True)
    hb = st.host_batch(st.tasks(), p)
    assert hb.contig_len is not None and set(hb.segments["svtype"].tolist()) == {0, 1, 2, 3, 4} and hb.segments["genotype"].all()
    off = hb.reads_off
    rng = np.random.default_rng(seed)
    rows0 = rng.permutation(int(off[1]))                  # contig 0: every row, out of order
    one = int(off[2]) + int(rng.integers(0, int(off[3] - off[2])))      # contig 2: one row
    rows = np.r_[rows0, one]
    reads = dict(reads_off=np.array([0, len(rows0), len(rows0), len(rows0) + 1], np.int64), r_start=hb.r_start[rows].astype(np.int32),
                 r_end=hb.r_end[rows].astype(np.int32), r_primary=hb.r_primary[rows].copy(), r_id=hb.r_id[rows].copy())
    assert len(rows0) > 100 and bool(np.any(np.diff(reads["r_start"][:len(rows0)]) < 0))
    return hb.segments, hb.a, hb.b, hb.read_id, hb.aux, hb.contig_len, reads


def with_device_reads(hb, rd):
    """the host batch `hb` with its four reads columns replaced by the device addresses of `rd` (reads.batch_columns):
    CSV_IN_READS_DEVICE on a batch whose signature columns stay host arrays"""
    assert hb.c.n_reads == rd["n_reads"] and np.array_equal(hb.reads_off, rd["reads_off"])
    hb.c.r_start, hb.c.r_end, hb.c.r_primary, hb.c.r_id = rd["r_start"], rd["r_end"], rd["r_primary"], rd["r_id"]
    hb.c.flags |= _abi.IN_READS_DEVICE
    return hb


RESULT_KEYS = ("call_seg", "call_cluster", "call_aux", "bp1", "bp2", "support", "cipos", "cilen", "search_pos", "seq_pick", "dr", "dv", "gl_idx", "support_off",
               "support_sig", "seg_status")


def assert_same_result(got, want):
    assert got["n_clusters"] == want["n_clusters"]
    for k in RESULT_KEYS:
        assert np.array_equal(got[k], want[k]), k


def raw(name, *args):
    """a csv_reads_* entry as it is -> the status"""
    return getattr(lib(), name)(*args)
