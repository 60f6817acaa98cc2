"""Helpers of test_index_build.py: the files whose index is built on every route, the refused files, and the twin - bai_writer's
bytes with its defaults, the checker of DESIGN.md section 30."""
import os

import numpy as np

import bai_writer
import bam_writer
import frame_helpers
import index_helpers

W = 16384
BIG = [("big", 1 << 29), ("small", 40_000)]


def rec(name, start, cigar, refid=0, flag=0, seq=None):
    qlen = sum(n for op, n in cigar if op in (0, 1, 4))
    return dict(name=name, flag=flag, mapq=30, start=start, cigar=cigar, seq=("ACGT" * (qlen // 4 + 1))[:qlen] if seq is None else seq, refid=refid)


def span_rec(name, start, span, refid=0):
    """a record of `span` reference bases, most of them under an N operation"""
    if span <= 20:
        return rec(name, start, [(0, span)], refid)
    gaps, left = [], span - 20
    while left > 0:                                           # (an operation's length has 28 bits)
        gaps.append((3, min(left, (1 << 28) - 1)))
        left -= gaps[-1][1]
    return rec(name, start, [(0, 10)] + gaps + [(0, 10)], refid)


def tail(n):
    return [dict(name="tail%d" % k, flag=4, mapq=0, start=-1, cigar=[], seq="ACGTAC", refid=-1) for k in range(n)]


def twin(path):
    """bai_writer's info of a BAM file (defaults: filled linear index, pseudo-bins, n_no_coor), with info["bytes"]"""
    with open(path, "rb") as f:
        info = bai_writer.build(f.read())
    info["bytes"] = bai_writer.to_bytes(info)
    return info


def twin_runs(info):
    """the chunks of the twin: one per maximal stretch of neighbours with one (refid, bin)"""
    return sum(len(c) for R in info["refs"] for c in R["bins"].values())


def level_records():
    """one record on each of the six bin levels of a reference of 2^29 bases, and one that ends exactly on 2^29"""
    out = [span_rec("l5", 100, 50), span_rec("l4", W - 400, 1000)]
    for k, shift in enumerate((17, 20, 23, 26)):
        out.append(span_rec("l%d" % (3 - k), (1 << shift) - 50, 100))
    out.append(span_rec("wide", 1 << 27, (1 << 29) - (1 << 27)))
    return out


def edge_files(tmp):
    """the crafted edges -> [(name, path)]"""
    out = []

    def add(name, refs, recs, **kw):
        path = str(tmp / (name + ".bam"))
        if not os.path.exists(path):
            bam_writer.write_bam(path, refs, recs, **kw)
        out.append((name, path))
    refs = index_helpers.REFS
    add("header_only", refs, [])
    add("tail_only", refs, tail(4))
    add("one_record", refs, [span_rec("a", 500, 80, 0), span_rec("only", 7000, 60, 1), span_rec("b", 9, 30, 2)])
    add("pos0", refs, [span_rec("z0", 0, 1), span_rec("z1", 0, 40), rec("neg", 0, [], flag=4, seq="ACGT")])
    add("window_edges", refs, [span_rec("ends_on", 3 * W - 100, 100), span_rec("starts_before", 3 * W - 1, 1), span_rec("crosses", 3 * W - 1, 2),
                               span_rec("ends_on2", 5 * W - 1, 1), span_rec("at", 5 * W, 1)], block_bytes=90)
    add("placed_unmapped", refs, [span_rec("m", 100, 50), rec("pu", 120, [], flag=4, seq="ACGTACGT"), rec("pu2", 120, [], flag=4 | 16, seq="AC"), span_rec("n", 130, 50)] + tail(2))
    add("levels", BIG, level_records() + [span_rec("s", 10, 10, 1)] + tail(1), block_bytes=150)
    # two same-bin neighbours, another bin, the first bin again: two chunks in that bin
    add("bin_again", refs, [span_rec("a1", 100, 50), span_rec("a2", 110, 50), span_rec("b1", 120, 20_000), span_rec("a3", 130, 50), span_rec("a4", 140, 50)], block_bytes=100)
    return out


def parity_files(tmp):
    """the files of the byte comparison -> [(name, path)]: the grid, the planted BAM, the grid at three block sizes with records on block
    boundaries, the CG placeholder form, stored blocks - and the crafted edges"""
    out = []
    grid = index_helpers.grid_records()

    def add(name, write):
        path = str(tmp / (name + ".bam"))
        if not os.path.exists(path):
            write(path)
            for ext in (".bai",):
                if os.path.exists(path + ext):
                    os.unlink(path + ext)
        out.append((name, path))
    add("grid", lambda p: index_helpers.write_grid_bam(p))
    add("planted", lambda p: index_helpers.write_planted_small_blocks(p))
    for bb in (64, 200, bam_writer.MAX_BLOCK):
        def write(p, bb=bb):
            info = bam_writer.write_bam(p, index_helpers.REFS, grid, block_bytes=bb)
            cuts = [info["records"][k]["offset"] for k in (0, 1, 40, 150, 151, 204, 333, 405, 409)] + [info["records"][409]["end"]]
            bam_writer.write_bam(p, index_helpers.REFS, grid, block_bytes=bb, cuts=cuts)
        add("grid_bb%d" % bb, write)
    add("grid_cg", lambda p: bam_writer.write_bam(p, index_helpers.REFS, grid, block_bytes=700, cg=True))
    add("grid_level0", lambda p: bam_writer.write_bam(p, index_helpers.REFS, grid, block_bytes=3000, level=0))
    # more records than one tile of the scan over the head flags holds (1 024), in one window
    add("many", lambda p: bam_writer.write_bam(p, frame_helpers.REFS, frame_helpers.short_records(2500, step=60)))
    return out + edge_files(tmp)


REFUSALS = {
    # name: (refs, records, the ordinal of the refused record, a piece of the text)
    "pos_2_29": ([("big", (1 << 29) + 1000)], [span_rec("ok", 100, 50), span_rec("far", 1 << 29, 10)], 1, "reaches 2^29 bases or beyond"),
    "end_2_29": ([("big", (1 << 29) + 1000)], [span_rec("ok", 100, 50), span_rec("over", (1 << 29) - 5, 6)], 1, "reaches 2^29 bases or beyond"),
    "beyond_reference": (index_helpers.REFS, [span_rec("ok", 100, 50), span_rec("ok2", 200, 50), span_rec("long", 1_999_990, 11)], 2, "ends beyond the length of its reference"),
    "pos_order": (index_helpers.REFS, [span_rec("r%d" % k, 1000 + 10 * k, 30) for k in range(70)] + [span_rec("back", 1500, 30)] + [span_rec("on", 1800, 30)], 70,
                  "is out of coordinate order"),
    "ref_order": (index_helpers.REFS, [span_rec("r%d" % k, 1000 + 10 * k, 30, 2) for k in range(5)] + [span_rec("back", 5000, 30, 0)], 5, "is out of coordinate order"),
    "mapped_after_tail": (index_helpers.REFS, [span_rec("a", 10, 30)] + tail(1) + [span_rec("b", 50, 30)], 2, "is out of coordinate order"),
}


def refusal_file(tmp, name, **kw):
    refs, recs, ordinal, text = REFUSALS[name]
    path = str(tmp / (name + ".bam"))
    bam_writer.write_bam(path, refs, recs, **kw)
    return path, ordinal, text


def same_stats(bf, info, names):
    """index_statistics / no_coordinate of a reader against the twin's counts"""
    want = [(n, R["n_mapped"], R["n_unmapped"], R["n_mapped"] + R["n_unmapped"]) for n, R in zip(names, info["refs"])]
    return bf.index_statistics() == want and bf.no_coordinate == info["n_no_coor"]


def expected_bytes_down(info, stats, lengths):
    """what a device build copies down when the rows stay on the device: one status byte per block the device inflated or gave up on (the
    blocks from the first record's on, each loaded once), 32 bytes of the stitch's verdict per framing run, 32 bytes of the index verdict per
    indexed window, 32 bytes per run row - a run cut by a window seam has one row in each window - and at the end the linear arrays
    and the counts"""
    n_lin = sum((min(max(int(l), 0), 1 << 29) >> 14) + 1 for l in lengths)
    return (stats["device_blocks"] + stats["fallback_blocks"] + 32 * stats["frame_runs"] + 32 * stats["index_windows"] + 32 * stats["runs"]
            + 8 * (n_lin + 2 * len(lengths) + 1))


def seam_rows(info, first_ordinals):
    """run rows a device build hands down: the twin's chunks, plus one for every window whose first record (ordinals given) carries on
    the run of the record before it"""
    recs = info["records"]
    extra = 0
    for o in first_ordinals:
        if o <= 0 or o >= len(recs) or recs[o]["refid"] < 0:
            continue
        a, b = recs[o - 1], recs[o]
        key = lambda r: (r["refid"], bam_writer.reg2bin(max(r["pos"], 0), max(r["end"], 1)))      # noqa: E731
        extra += key(a) == key(b)
    return twin_runs(info) + extra


def rng_bytes(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
