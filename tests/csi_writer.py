"""A CSI index (.csi) writer for the tests, from the format as DESIGN.md section 32 and cutesv_amd/csrc/csi_index.h restate it, with
`struct` and `zlib` only.  It reads a written BAM with bai_writer's BGZF walk and imports no product code, so the parser and the build
under test and this writer are two independent readings of the format that check each other - the part bai_writer.py plays for BAI.

    info = write_csi("x.bam")                        # writes x.bam.csi; min_shift=14, depth=None: htslib's rule

info: dict(min_shift, depth, n_ref, lengths, refs=[dict(n_mapped, n_unmapped, beg, end, bins={bin: [(beg, end), ...]}, loff={bin:
loffset}, lin={window: smallest voff})], n_no_coor, blocks, records, payload, bytes) - what the file says, for the tests to compare with.
"""
import bisect
import struct
import zlib

import bai_writer

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_BLOCK = 0xFF00


def first(level):
    """the number of the first bin of a level (0: the root)"""
    return ((1 << 3 * level) - 1) // 7


def n_bins(depth):
    return first(depth + 1)


def pseudo_bin(depth):
    return n_bins(depth) + 1


def reg2bin(beg, end, min_shift, depth):
    """the deepest bin that holds both beg and end - 1"""
    end -= 1
    for level in range(depth, 0, -1):
        shift = min_shift + 3 * (depth - level)
        if beg >> shift == end >> shift:
            return first(level) + (beg >> shift)
    return 0


def level_of(b, depth):
    return max(lv for lv in range(depth + 1) if first(lv) <= b)


def bot(b, depth):
    """the first window of the deepest level that bin b holds"""
    lv = level_of(b, depth)
    return (b - first(lv)) << 3 * (depth - lv)


def auto_depth(lengths, min_shift):
    """htslib's rule: the smallest depth with max(l_ref) + 256 <= 2^(min_shift + 3 * depth)"""
    need, depth = max(list(lengths) + [0]) + 256, 0
    while need > 1 << (min_shift + 3 * depth):
        depth += 1
    return depth


def read_lengths(stream):
    l_text, = struct.unpack_from("<i", stream, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, o)
    o += 4
    out = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, o)
        out.append(struct.unpack_from("<i", stream, o + 4 + l_name)[0])
        o += 8 + l_name
    return out


def build(blob, min_shift=14, depth=None):
    blocks, stream = bai_writer.read_blocks(blob)
    n_ref, recs = bai_writer.read_records(stream)
    lengths = read_lengths(stream)
    if depth is None:
        depth = auto_depth(lengths, min_shift)
    ustart, u = [], 0
    for _, _, isize in blocks:
        ustart.append(u)
        u += isize
    refs = [dict(n_mapped=0, n_unmapped=0, bins={}, loff={}, lin={}, beg=None, end=None) for _ in range(n_ref)]
    n_no_coor = 0
    for r in recs:
        r["voff"] = bai_writer._voff(blocks, ustart, r["off"])
        r["voff_end"] = bai_writer._voff(blocks, ustart, r["off_end"]) if r["off_end"] < len(stream) else blocks[-1][0] << 16
        if r["refid"] < 0:
            n_no_coor += 1
            continue
        R = refs[r["refid"]]
        R["n_unmapped" if r["flag"] & 4 else "n_mapped"] += 1
        if R["beg"] is None:
            R["beg"] = r["voff"]
        R["end"] = r["voff_end"]
        beg, end = max(r["pos"], 0), max(r["end"], 1)
        assert end <= 1 << (min_shift + 3 * depth), "the record reaches beyond what (%d, %d) indexes" % (min_shift, depth)
        chunks = R["bins"].setdefault(reg2bin(beg, end, min_shift, depth), [])
        if chunks and chunks[-1][1] == r["voff"]:             # neighbours of one bin: one chunk
            chunks[-1] = (chunks[-1][0], r["voff_end"])
        else:
            chunks.append((r["voff"], r["voff_end"]))
        for w in range(beg >> min_shift, ((end - 1) >> min_shift) + 1):
            if w not in R["lin"] or r["voff"] < R["lin"][w]:
                R["lin"][w] = r["voff"]
    for R in refs:                                            # loffset: the entry of the first touched window at or behind bot(bin)
        touched = sorted(R["lin"])
        for b in R["bins"]:
            k = bisect.bisect_left(touched, bot(b, depth))
            R["loff"][b] = R["lin"][touched[k]] if k < len(touched) else 0
    return dict(min_shift=min_shift, depth=depth, n_ref=n_ref, lengths=lengths, refs=refs, n_no_coor=n_no_coor, blocks=blocks, records=recs)


def to_payload(info, pseudo=True, no_coor=True):
    out = [b"CSI\1", struct.pack("<iiii", info["min_shift"], info["depth"], 0, info["n_ref"])]
    for R in info["refs"]:
        bins = sorted(R["bins"].items())
        has_pseudo = pseudo and R["beg"] is not None
        out.append(struct.pack("<i", len(bins) + (1 if has_pseudo else 0)))
        for b, chunks in bins:
            out.append(struct.pack("<IQi", b, R["loff"][b], len(chunks)))
            out.extend(struct.pack("<QQ", c0, c1) for c0, c1 in chunks)
        if has_pseudo:
            out.append(struct.pack("<IQiQQQQ", pseudo_bin(info["depth"]), 0, 2, R["beg"], R["end"], R["n_mapped"], R["n_unmapped"]))
    if no_coor:
        out.append(struct.pack("<Q", info["n_no_coor"]))
    return b"".join(out)


def bgzf_block(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    return (struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def compress(payload, block_bytes=MAX_BLOCK, eof=True):
    """the payload as a .csi file holds it: BGZF blocks and the end-of-file block"""
    return b"".join(bgzf_block(payload[a : a + block_bytes]) for a in range(0, len(payload), block_bytes)) + (EOF_BLOCK if eof else b"")


def write_payload(path, payload, **kw):
    with open(path, "wb") as f:
        f.write(compress(payload, **kw))
    return str(path)


def write_csi(bam_path, csi_path=None, min_shift=14, depth=None, pseudo=True, no_coor=True, block_bytes=MAX_BLOCK):
    with open(bam_path, "rb") as f:
        info = build(f.read(), min_shift, depth)
    info["payload"] = to_payload(info, pseudo=pseudo, no_coor=no_coor)
    info["bytes"] = compress(info["payload"], block_bytes)
    info["path"] = csi_path or str(bam_path) + ".csi"
    with open(info["path"], "wb") as f:
        f.write(info["bytes"])
    return info


def fields(payload):
    """a second walk, over the payload: [dict(ref, bin, at (offset of the bin number), loffset, n_chunk, chunks_at)] and the offset
    behind the last reference - for the tests that damage single fields"""
    assert payload[:4] == b"CSI\1"
    l_aux, = struct.unpack_from("<i", payload, 12)
    n_ref, = struct.unpack_from("<i", payload, 16 + l_aux)
    o, out, n_bin_at = 20 + l_aux, [], []
    for r in range(n_ref):
        n_bin_at.append(o)
        n_bin, = struct.unpack_from("<i", payload, o)
        o += 4
        for _ in range(n_bin):
            b, lo, n_chunk = struct.unpack_from("<IQi", payload, o)
            out.append(dict(ref=r, bin=b, at=o, loffset=lo, n_chunk=n_chunk, chunks_at=o + 16))
            o += 16 + 16 * n_chunk
    return dict(bins=out, n_bin_at=n_bin_at, end_refs=o, n_ref_at=16 + l_aux)


def read_payload(payload):
    """a payload -> dict(min_shift, depth, refs=[dict(bins={bin: (loffset, [(beg, end), ...])}, pseudo=(beg, end, n_mapped, n_unmapped) or
    None)], n_no_coor (None: absent)) - the pseudo-bin told from the regular ones by its number"""
    assert payload[:4] == b"CSI\1"
    min_shift, depth, l_aux = struct.unpack_from("<iii", payload, 4)
    n_ref, = struct.unpack_from("<i", payload, 16 + l_aux)
    o, refs = 20 + l_aux, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", payload, o)
        o += 4
        R = dict(bins={}, pseudo=None, order=[])
        for _ in range(n_bin):
            b, lo, n_chunk = struct.unpack_from("<IQi", payload, o)
            chunks = [struct.unpack_from("<QQ", payload, o + 16 + 16 * k) for k in range(n_chunk)]
            o += 16 + 16 * n_chunk
            R["order"].append(b)
            if b == pseudo_bin(depth):
                assert n_chunk == 2 and lo == 0
                R["pseudo"] = chunks[0] + chunks[1]
            else:
                R["bins"][b] = (lo, chunks)
        refs.append(R)
    n_no_coor = struct.unpack_from("<Q", payload, o)[0] if o < len(payload) else None
    assert o + (8 if n_no_coor is not None else 0) == len(payload)
    return dict(min_shift=min_shift, depth=depth, refs=refs, n_no_coor=n_no_coor)
