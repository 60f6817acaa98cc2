"""A BAM index (.bai) writer for the tests, from the SAM specification (SAMv1 sections 4.1 BGZF, 4.2 BAM, 5.2 "The BAI index format",
5.3 "C source code for computing bin number") with `struct` and `zlib` only.  It reads a written BAM with a BGZF walk of its own:
no product code is imported (the bin of a region is bam_writer.reg2bin), so the parser under test (cutesv_amd/csrc/bai_index.h)
and this writer are two independent readings of the specification that check each other, as bam_writer.py and the reader do.

    info = write_bai("x.bam")                       # writes x.bam.bai

info: dict(n_ref, refs=[dict(n_mapped, n_unmapped, ioffset=[...], bins={bin: [(beg, end), ...]})], n_no_coor, blocks=[(coffset,
csize, isize)], records=[dict(refid, pos, end, flag, voff, voff_end)]) - what the file says, for the tests to compare with.

fill: True - an empty window of the linear index takes the entry of the next window that has one, as htslib writes it; False - it
stays 0, as old samtools left it.  block_end: True - a record that starts on a block boundary gets the virtual offset (that block,
ISIZE) instead of (next block, 0); both name the same byte.  pseudo / no_coor: write the pseudo-bins / the trailing n_no_coor.
"""
import struct
import zlib

from bam_writer import reg2bin

PSEUDO_BIN = 37450
_REF_OPS = (0, 2, 3, 7, 8)


def read_blocks(blob):
    """the BGZF blocks of a file's bytes -> ([(coffset, csize, isize)], the inflated stream)"""
    blocks, parts, o = [], [], 0
    while o < len(blob):
        assert blob[o : o + 4] == b"\x1f\x8b\x08\x04", "not a BGZF block at byte %d" % o
        xlen, = struct.unpack_from("<H", blob, o + 10)
        x, bsize = 0, None
        while x + 4 <= xlen:
            si, slen = blob[o + 12 + x : o + 14 + x], struct.unpack_from("<H", blob, o + 14 + x)[0]
            if si == b"BC" and slen == 2:
                bsize, = struct.unpack_from("<H", blob, o + 16 + x)
            x += 4 + slen
        assert bsize is not None
        total = bsize + 1
        data = zlib.decompress(blob[o + 12 + xlen : o + total - 8], -15)
        crc, isize = struct.unpack_from("<II", blob, o + total - 8)
        assert len(data) == isize and zlib.crc32(data) & 0xFFFFFFFF == crc
        blocks.append((o, total, isize))
        parts.append(data)
        o += total
    return blocks, b"".join(parts)


def read_records(stream):
    """the inflated stream of a BAM -> (n_ref, [dict(refid, pos, end, flag, off, off_end)]): end = pos + max(reference span, 1)"""
    assert stream[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", stream, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, o)
        o += 8 + l_name
    recs = []
    while o < len(stream):
        bs, = struct.unpack_from("<i", stream, o)
        refid, pos, l_name, _mapq, _bin, n_cig, flag, _l_seq = struct.unpack_from("<iiBBHHHI", stream, o + 4)
        cig = struct.unpack_from("<%dI" % n_cig, stream, o + 36 + l_name)
        span = sum(w >> 4 for w in cig if w & 15 in _REF_OPS)
        recs.append(dict(refid=refid, pos=pos, end=pos + max(span, 1), flag=flag, off=o, off_end=o + 4 + bs))
        o += 4 + bs
    return n_ref, recs


def _voff(blocks, ustart, u, block_end=False):
    """the virtual offset of byte u of the inflated stream (ustart[k]: where block k's bytes begin)"""
    lo, hi = 0, len(blocks)
    while hi - lo > 1:
        m = (lo + hi) // 2
        if ustart[m] <= u:
            lo = m
        else:
            hi = m
    while lo + 1 < len(blocks) and blocks[lo][2] == 0:       # (an empty block holds no byte)
        lo += 1
    if block_end and lo > 0 and ustart[lo] == u:
        k = lo - 1
        while k > 0 and blocks[k][2] == 0:
            k -= 1
        if blocks[k][2]:
            return blocks[k][0] << 16 | blocks[k][2]
    return blocks[lo][0] << 16 | (u - ustart[lo])


def build(blob, fill=True, block_end=False):
    blocks, stream = read_blocks(blob)
    n_ref, recs = read_records(stream)
    ustart, u = [], 0
    for _, _, isize in blocks:
        ustart.append(u)
        u += isize
    refs = [dict(n_mapped=0, n_unmapped=0, ioffset=[], bins={}, beg=None, end=None) for _ in range(n_ref)]
    n_no_coor = 0
    for r in recs:
        r["voff"] = _voff(blocks, ustart, r["off"], block_end)
        r["voff_end"] = _voff(blocks, ustart, r["off_end"]) if r["off_end"] < len(stream) else blocks[-1][0] << 16
        if r["refid"] < 0:
            n_no_coor += 1
            continue
        R = refs[r["refid"]]
        R["n_unmapped" if r["flag"] & 4 else "n_mapped"] += 1
        if R["beg"] is None:
            R["beg"] = r["voff"]
        R["end"] = r["voff_end"]
        beg, end = max(r["pos"], 0), max(r["end"], 1)
        chunks = R["bins"].setdefault(reg2bin(beg, end), [])
        if chunks and chunks[-1][1] == r["voff"]:             # neighbours of one bin: one chunk
            chunks[-1] = (chunks[-1][0], r["voff_end"])
        else:
            chunks.append((r["voff"], r["voff_end"]))
        io = R["ioffset"]
        w0, w1 = beg >> 14, (end - 1) >> 14
        io.extend([0] * (w1 + 1 - len(io)))
        for w in range(w0, w1 + 1):
            if io[w] == 0 or r["voff"] < io[w]:
                io[w] = r["voff"]
    if fill:
        for R in refs:
            io = R["ioffset"]
            for w in range(len(io) - 2, -1, -1):
                if io[w] == 0:
                    io[w] = io[w + 1]
    return dict(n_ref=n_ref, refs=refs, n_no_coor=n_no_coor, blocks=blocks, records=recs)


def to_bytes(info, pseudo=True, no_coor=True):
    out = [b"BAI\1", struct.pack("<i", info["n_ref"])]
    for R in info["refs"]:
        bins = sorted(R["bins"].items())
        has_pseudo = pseudo and R["beg"] is not None
        out.append(struct.pack("<i", len(bins) + (1 if has_pseudo else 0)))
        for b, chunks in bins:
            out.append(struct.pack("<Ii", b, len(chunks)))
            out.extend(struct.pack("<QQ", c0, c1) for c0, c1 in chunks)
        if has_pseudo:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["beg"], R["end"], R["n_mapped"], R["n_unmapped"]))
        out.append(struct.pack("<i", len(R["ioffset"])))
        out.extend(struct.pack("<Q", v) for v in R["ioffset"])
    if no_coor:
        out.append(struct.pack("<Q", info["n_no_coor"]))
    return b"".join(out)


def write_bai(bam_path, bai_path=None, fill=True, block_end=False, pseudo=True, no_coor=True):
    with open(bam_path, "rb") as f:
        blob = f.read()
    info = build(blob, fill=fill, block_end=block_end)
    info["bytes"] = to_bytes(info, pseudo=pseudo, no_coor=no_coor)
    info["path"] = bai_path or str(bam_path) + ".bai"
    with open(info["path"], "wb") as f:
        f.write(info["bytes"])
    return info


def field_offsets(data):
    """a second walk, over the index bytes: {"n_ref": off, "n_bin": [off per ref], "n_chunk": [off per bin], "n_intv": [off per ref],
    "ioffset": [(off, n) per ref], "end_refs": off} - where the count fields are, for the tests that damage them"""
    assert data[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", data, 4)
    out, o = dict(n_ref=4, n_bin=[], n_chunk=[], n_intv=[], ioffset=[]), 8
    for _ in range(n_ref):
        out["n_bin"].append(o)
        n_bin, = struct.unpack_from("<i", data, o)
        o += 4
        for _ in range(n_bin):
            out["n_chunk"].append(o + 4)
            n_chunk, = struct.unpack_from("<i", data, o + 4)
            o += 8 + 16 * n_chunk
        out["n_intv"].append(o)
        n_intv, = struct.unpack_from("<i", data, o)
        out["ioffset"].append((o + 4, n_intv))
        o += 4 + 8 * n_intv
    out["end_refs"] = o
    return out
