"""Helpers of test_bam_frame.py: the small files both the CPU twin and the GPU tests read, the decoy records, the windows the reader
forms over a file, and the corpus format of tests/frame_core_main.cpp."""
import struct
import zlib

import numpy as np

import bam_writer

REFS = [("7", 5_000_000), ("X", 1_000_000)]
_LETTERS = "=ACMGRSVTWYHKDBN"


def short_records(n, seed=3, refid=0, start=1000, step=40, name="r%04d", tags=True):
    """n short records, sorted: a few CIGAR operations, 20 - 60 bases, an NM tag and now and then an SA tag"""
    rng = np.random.RandomState(seed)
    recs, pos = [], start
    for k in range(n):
        m = int(rng.randint(10, 30))
        ops = [(4, int(rng.randint(1, 9))), (0, m), (1, int(rng.randint(1, 6))), (0, int(rng.randint(5, 20)))]
        qlen = sum(ln for op, ln in ops if op in (0, 1, 4))
        t = [("NM", int(rng.randint(0, 9)))] + ([("SA", "X,%d,+,10S20M,30,1;" % (100 + k))] if k % 5 == 0 else []) if tags else []
        recs.append(dict(name=name % k, flag=(0, 16, 256, 2048)[k % 4], mapq=int(rng.randint(0, 61)), start=pos, cigar=ops,
                         seq="".join("ACGT"[i] for i in rng.randint(0, 4, qlen)), tags=t, refid=refid))
        pos += int(rng.randint(0, step))
    return recs


def minimal_records(n, refid=0):
    """n records of the smallest kind: a one-letter name, no CIGAR, no bases, no tag (block_size 34)"""
    return [dict(name="m", flag=4, mapq=0, start=10 + k, cigar=[], seq="", tags=[], refid=refid) for k in range(n)]


def fake_chain():
    """the bytes of three well-formed little records back to back: what a decoy carries"""
    return b"".join(bam_writer.record_bytes(dict(name="fake%d" % k, flag=0, mapq=9, start=77 + k, cigar=[(0, 8)], seq="ACGTACGT", tags=[("NM", k)], refid=0))[0]
                    for k in range(3))


def seq_of_bytes(data):
    """the base letters whose 4-bit packing is `data`"""
    return "".join(_LETTERS[b >> 4] + _LETTERS[b & 15] for b in data)


def decoy_file(path, block_bytes=bam_writer.MAX_BLOCK):
    """short records, of which one carries the fake chain in a B:C array and one in its sequence bytes; block boundaries stand at the
    first byte of either chain -> (info, the number of planted blocks)"""
    recs = short_records(40, seed=9)
    chain = fake_chain()
    recs[10] = dict(recs[10], tags=[("XD", "B", ("C", list(chain)))])
    recs[25] = dict(recs[25], seq=seq_of_bytes(chain), cigar=[(0, 2 * len(chain))])
    info = bam_writer.write_bam(path, REFS, recs)
    cuts = [info["records"][10]["aux"] + 8, info["records"][25]["seq"]]
    return bam_writer.write_bam(path, REFS, recs, cuts=cuts, block_bytes=block_bytes), 2


def inside_cuts(info, k):
    """block boundaries on record k's start, 1, 2 and 3 bytes into its block_size word, and inside each of its parts"""
    r = info["records"][k]
    return [r["offset"], r["offset"] + 1, r["offset"] + 2, r["offset"] + 3, r["fixed"] + 13, r["name"] + 2, r["cigar"] + 5, r["seq"] + 3, r["qual"] + 4, r["aux"] + 2]


def plain_files(tmp, write=True):
    """[(path, window_blocks)] of the plain files of the GPU parity tests (written once per directory)"""
    recs = short_records(300)
    out = []

    def add(name, rs, wb=0, **kw):
        path = str(tmp / name)
        if write:
            bam_writer.write_bam(path, REFS, rs, **kw)
        out.append((path, wb))
    base = bam_writer.write_bam(str(tmp / "_probe.bam"), REFS, recs)
    cuts = sum((inside_cuts(base, k) for k in (3, 50, 120, 299)), [])
    for bb in (64, 200, 4096, bam_writer.MAX_BLOCK):
        add("bb%d.bam" % bb, recs, wb=(1, 2, 64, 0)[(bb // 64) % 4], block_bytes=bb)
        add("cut%d.bam" % bb, recs, wb=(0, 64, 2, 1)[(bb // 64) % 4], block_bytes=bb, cuts=cuts)
    add("records.bam", recs, cuts="record")
    add("empty.bam", [dict(r, refid=1) for r in recs[:5]])
    add("one.bam", recs[:1])
    long_one = dict(recs[7], seq="ACGT" * 300, cigar=[(0, 1200)])           # a record that spans more than three blocks of 200 bytes
    add("span.bam", recs[:7] + [long_one] + recs[8:40], wb=1, block_bytes=200)
    add("span2.bam", recs[:7] + [long_one] + recs[8:40], wb=2, block_bytes=200)
    add("min64.bam", minimal_records(64))
    add("min65.bam", minimal_records(65))
    add("two.bam", [dict(r, refid=0) for r in recs[:100]] + [dict(r, refid=1) for r in recs[100:200]] +
        [dict(r, refid=-1, start=-1, cigar=[], flag=4, mapq=0, tags=[]) for r in recs[200:207]], wb=2, block_bytes=3000)
    return out


def stream_of(path):
    """a BGZF file -> (its inflated bytes, the ISIZE of every block)"""
    blob = open(path, "rb").read()
    data, lens, o = [], [], 0
    while o < len(blob):
        size = struct.unpack_from("<H", blob, o + 16)[0] + 1
        d = zlib.decompress(blob[o + 18 : o + size - 8], -15)
        data.append(d); lens.append(len(d))
        o += size
    return b"".join(data), lens


def header_end(stream):
    l_text = struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, 8 + l_text)[0]
    o = 12 + l_text
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", stream, o)[0]
    return o, n_ref


def naive_walk(w, c):
    """the chain of record starts of the window `w` from c -> (starts, tail): the walk the core must reproduce"""
    starts, o = [], c
    while o + 4 <= len(w):
        bs = struct.unpack_from("<i", w, o)[0]
        if bs < 32 or o + 4 + bs > len(w):
            break
        starts.append(o)
        o += 4 + bs
    return starts, o


def windows_of(stream, lens, window_blocks=4096):
    """the windows the reader forms over a file read from its first record to its end: [(bytes, block lengths, cursor)]"""
    off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    cur, _ = header_end(stream)
    nb, out = len(lens), []
    while cur < len(stream):
        b0 = int(np.searchsorted(off, cur, side="right") - 1)
        while b0 + 1 < nb and lens[b0] == 0:
            b0 += 1
        b1 = min(nb, b0 + window_blocks)
        need = 4
        if cur + 4 <= len(stream):
            bs = struct.unpack_from("<i", stream, cur)[0]
            need = 4 + max(bs, 0)
        while b1 < nb and off[b1] < cur + need:
            b1 += 1
        w = stream[int(off[b0]) : int(off[b1])]
        c = cur - int(off[b0])
        out.append((w, list(lens[b0:b1]), c))
        _, tail = naive_walk(w, c)
        if tail == c:
            break
        cur = int(off[b0]) + tail
    return out


def write_corpus(path, windows, n_ref):
    """the corpus file of frame_core_main: windows = [(bytes, block lengths, cursor)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(windows)))
        for w, lens, c in windows:
            f.write(struct.pack("<IiII", len(w), n_ref, len(lens), c))
            f.write(struct.pack("<%dI" % len(lens), *lens))
            f.write(w)


def rows_hash(w, starts):
    """FNV-1a over the 40-byte rows (frame_core.h's FrRow) of the records at `starts` of the window `w`: what frame_core_main prints"""
    h = 1469598103934665603
    for o in starts:
        bs, refid, pos = struct.unpack_from("<iii", w, o)
        l_name, n_cig, l_seq = w[o + 12], struct.unpack_from("<H", w, o + 16)[0], struct.unpack_from("<I", w, o + 20)[0]
        cg, end = o + 36 + l_name, o + 4 + bs
        n_in = min(n_cig, max(0, (end - cg) // 4))
        ops = np.frombuffer(w, "<u4", n_in, cg) if n_in else np.zeros(0, np.uint32)
        span = int((ops >> 4)[np.isin(ops & 15, (0, 2, 3, 7, 8))].sum(dtype=np.int64))
        for b in struct.pack("<qqiiiIHBBI", o, span, bs, refid, pos, l_seq, n_cig, l_name, 0, 0):
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
