"""Helpers of the CSI tests (test_csi_index.py, test_csi_build.py): a BAM writer for positions at and beyond 2^29, where
bam_writer.py cannot pack the BAI bin - the same record layout with the record's own bin field set to the low 16 bits of the bin, a
field nothing in the reader reads - and the files the tests share."""
import os
import struct

import bam_writer
import csi_writer
from index_build_helpers import rec, span_rec, tail

P29 = 1 << 29
L600 = 600_000_000
BIG_REFS = [("huge", L600), ("also", L600)]
W = 16384
ALL = 1 << 62


def record_bytes(r):
    """bam_writer.record_bytes for any position an int32 holds"""
    name = r["name"].encode() + b"\0"
    cigar = [(int(op), int(ln)) for op, ln in r["cigar"]]
    seq = r["seq"]
    l_seq = len(seq)
    ref_len = sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
    start = int(r["start"])
    codes = seq.encode().translate(bam_writer._SEQ_TABLE) + b"\0"
    packed = bytes(hi << 4 | lo for hi, lo in zip(codes[0:l_seq:2], codes[1 : l_seq + 1 : 2]))
    own_bin = csi_writer.reg2bin(max(start, 0), max(start, 0) + max(ref_len, 1), 14, 6) & 0xFFFF
    body = struct.pack("<iiBBHHHIiii", r.get("refid", 0), start, len(name), r["mapq"], own_bin, len(cigar), r["flag"], l_seq, -1, -1, 0)
    blob = b"".join([body, name, struct.pack("<%dI" % len(cigar), *[ln << 4 | op for op, ln in cigar]), packed, b"\xff" * l_seq])
    return struct.pack("<i", len(blob)) + blob


def write_bam(path, refs, records, block_bytes=bam_writer.MAX_BLOCK, cut_before=()):
    """bam_writer.write_bam's file for such records -> the offsets of the records in the inflated stream.  cut_before: ordinals of
    records that start a BGZF block (the first record always does: the header has blocks of its own)"""
    text = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in refs)).encode()
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, ln in refs:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    parts, offs, o = [head], [], len(head)
    for r in records:
        parts.append(record_bytes(r))
        offs.append(o)
        o += len(parts[-1])
    data = b"".join(parts)
    step = min(block_bytes, bam_writer.MAX_BLOCK)
    points = sorted({len(head)} | {offs[k] for k in cut_before}) if offs else []
    out, a = [], 0
    for b in points + [len(data)]:
        while a < b:
            e = min(b, a + step)
            out.append(bam_writer.bgzf_block(data[a:e]))
            a = e
    with open(path, "wb") as f:
        f.write(b"".join(out) + bam_writer.EOF_BLOCK)
    return offs


def big_records():
    """two contigs of 600 Mbp: records in front of, around and far behind 2^29, long ones that hold the 128 kb and higher bins, a
    stretch of many short ones (many blocks) and a record that ends on the contig's last base"""
    out = []
    for refid in (0, 1):
        n = "c%d_" % refid
        out += [span_rec(n + "first", 50, 100, refid), span_rec(n + "long_low", 3 * W + 5, 300_000, refid)]
        out += [span_rec(n + "low%03d" % k, 40 * W + 97 * k, 60, refid) for k in range(150)]
        out += [span_rec(n + "reach", P29 - 5 * W, 4 * W + 100, refid), span_rec(n + "before", P29 - 1, 1, refid), span_rec(n + "cross", P29 - 1, 2, refid),
                span_rec(n + "at", P29, 1, refid), span_rec(n + "at_long", P29, 200_000, refid)]
        out += [span_rec(n + "hi%03d" % k, P29 + 30 * W + 131 * k, 80, refid) for k in range(200)]
        out += [span_rec(n + "far", 580_000_000, 70, refid), span_rec(n + "far2", 580_000_000 + 3 * W, 1_000_000, refid), span_rec(n + "far3", 580_000_000 + 9 * W + 7, 50, refid),
                span_rec(n + "last", L600 - 1, 1, refid)]
    return out + tail(3)


def write_big(path, block_bytes=700):
    recs = big_records()
    if not os.path.exists(path):
        write_bam(path, BIG_REFS, recs, block_bytes=block_bytes)
    return recs


def big_points():
    """region bounds of the read grid on a 600 Mbp contig"""
    pts = {0, 1, 50, 3 * W, 3 * W + 5, 22 * W, 40 * W - 1, 40 * W, 41 * W + 3, 100 * W, P29 - 5 * W, P29 - W, P29 - 1, P29, P29 + 1, P29 + 13 * W, P29 + 30 * W, P29 + 31 * W + 9,
           P29 + 40 * W, 570_000_000, 580_000_000, 580_000_000 + 3 * W, 580_000_000 + 9 * W + 7, 580_000_000 + 70 * W, L600 - 1, L600, L600 + 5}
    return sorted(pts)


def ref_span(r):
    return max(sum(n for op, n in r["cigar"] if op in (0, 2, 3, 7, 8)), 1)


def fresh(bf):
    bf.set_inflate(None)                                                    # (drops the inflated window: every read pays for its own blocks)


def check_read_grid(ix, fw, recs):
    """section 28's contract on a CSI-backed reader `ix` of the 600 Mbp file against the forward scan `fw`, both on the host routes"""
    import index_helpers as ih
    n_checked = n_less = 0
    for refid, chrom in enumerate(ix.references):
        pairs = list(ih.grid_pairs(big_points(), L600)) + [(-ALL, ALL), (0, L600), (P29 - 1, P29), (P29, P29 + 1), (L600 - 1, L600)]
        for beg, end in pairs:
            fresh(ix); fresh(fw)
            a, b = ix.records(chrom, beg, end), fw.records(chrom, beg, end)
            assert ih.same_chunk(a, b), (chrom, beg, end, a.n, b.n)
            want = [r["name"] for r in recs if r.get("refid", 0) == refid and r["start"] < end and r["start"] + ref_span(r) > beg]
            assert [a.name(i) for i in range(a.n)] == want, (chrom, beg, end)
            assert a.stats["compressed_bytes"] <= b.stats["compressed_bytes"], (chrom, beg, end)
            n_less += a.stats["compressed_bytes"] < b.stats["compressed_bytes"]
            n_checked += 1
    assert n_checked > 150 and n_less > 60
    for beg in (P29 - 1, P29, L600 - 1):                                        # each of the three is covered, and found
        fresh(ix)
        assert ix.records("also", beg, beg + 1).n >= 1


# ---- the files of the device build (test_csi_build.py)
COUNTS = (1, 63, 64, 65, 257)


def _run_of(n, start, refid, name):
    return [span_rec("%s%03d" % (name, k), start + k, 30, refid) for k in range(n)]


def build_files(tmp):
    """[(name, path, (min_shift, depth) or None for htslib's rule)] - what each file is for is in its name"""
    out = []

    def add(name, refs, recs, fmt=None, block_bytes=600, cut_before=()):
        path = str(tmp / (name + ".bam"))
        if not os.path.exists(path):
            write_bam(path, refs, recs, block_bytes=block_bytes, cut_before=cut_before)
        out.append((name, path, fmt))
    two31 = [("max", (1 << 31) - 1), ("small", 40_000)]
    # span 1 at 2^29 - 1, 2^29 and 2^31 - 2; a record crossing 2^29; unmapped records with coordinates; a tail
    edges = [span_rec("a", P29 - 1, 1), rec("pu", P29 - 1, [], flag=4, seq="ACGT"), span_rec("x", P29 - 1, 2), span_rec("b", P29, 1), rec("pu2", P29 + 7, [], flag=4 | 16, seq="AC"),
             span_rec("c", (1 << 31) - 2, 1), span_rec("s", 10, 10, 1)] + tail(2)
    add("edges_auto", two31, edges)
    add("edges_14_6", two31, edges, (14, 6))
    add("edges_12_7", two31, edges, (12, 7))
    # records that span 1, 4, 5, 68 and 70 windows: the lane path, the wavefront path, more than 64 shared windows
    spans = [span_rec("w%d" % n, P29 - 2 * W + 50 * k + 1, (n - 1) * W + 2 if n > 1 else 5) for k, n in enumerate((1, 4, 5, 68, 70))]
    add("spans_14_6", BIG_REFS, spans, (14, 6))
    spans12 = [span_rec("w%d" % n, 9 * 4096 + 50 * k + 1, (n - 1) * 4096 + 2 if n > 1 else 5) for k, n in enumerate((1, 4, 5, 68, 70))]
    add("spans_12_6", [("r", 900_000_000), ("q", 5000)], spans12 + [span_rec("q", 7, 9, 1)], (12, 6))
    # index windows of 1, 63, 64, 65 and 257 records: one BGZF block each, which a reader with windows of one block indexes one by one
    many, cuts = [], []
    for k, n in enumerate(COUNTS):
        cuts.append(len(many))
        many += _run_of(n, P29 + (10 + 7 * k) * W, 0, "m%d_" % n)
    cuts.append(len(many))
    add("counts_14_6", BIG_REFS, many + tail(1), (14, 6), block_bytes=bam_writer.MAX_BLOCK, cut_before=cuts)
    add("counts_14_5", [("r", P29), ("q", 5000)], [dict(r, start=r["start"] - P29) for r in many], (14, 5), block_bytes=bam_writer.MAX_BLOCK, cut_before=cuts[:-1])
    # three references inside one wavefront, with an empty reference between them
    refs4 = [("a", L600), ("empty", 1000), ("b", 70_000), ("c", L600)]
    three = _run_of(20, L600 - 100, 0, "a") + _run_of(20, 5, 2, "b") + _run_of(20, P29 + 3, 3, "c")
    add("three_refs", refs4, three)
    add("big_grid", BIG_REFS, big_records(), None, block_bytes=700)
    return out


REFUSALS = {
    # name: (refs, records, (min_shift, depth), the ordinal of the refused record, a piece of the text)
    "order": (BIG_REFS, [span_rec("a", P29 + 100, 30), span_rec("b", P29 + 200, 30), span_rec("back", P29 + 150, 30)], (14, 6), 2, "is out of coordinate order"),
    "beyond_l_ref": (BIG_REFS, [span_rec("a", P29 + 100, 30), span_rec("over", L600 - 5, 6)], (14, 6), 1, "ends beyond the length of its reference"),
    "beyond_max_pos": (BIG_REFS, [span_rec("a", 100, 30), span_rec("x", P29 - 1, 2)], (14, 5), 1,
                       "reaches 2^29 bases or beyond, which a CSI index with min_shift 14 and depth 5 cannot index"),
    "beyond_max_pos_12": (BIG_REFS, [span_rec("a", 100, 30), span_rec("x", 1 << 27, 1)], (12, 5), 1,
                          "reaches 2^27 bases or beyond, which a CSI index with min_shift 12 and depth 5 cannot index"),
}
