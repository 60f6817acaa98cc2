"""A small BAM writer for the tests, from the SAM/BAM specification (SAMv1 sections 4.1 BGZF, 4.2 BAM) with `struct` and
`zlib` only.  It shares no code with the reader under test (cutesv_amd.bam is not imported): no htslib-made file exists in
the test environment, so the two independent readings of the specification check each other.

    info = write_bam(path, [("7", 159345973)], records, cuts="record")

records: dicts `name, flag, mapq, start, cigar [(op, len)], seq, tags [(key, value) | (key, type, value)], refid`
(refid defaults to 0; -1 with start -1 for the unmapped tail).  A CIGAR of more than 65 535 operations (or cg=True) is
written as the `<l_seq>S<reference length>N` placeholder with the real operations in a CG:B,I tag (4.2.2).
cuts: where BGZF blocks end, as offsets into the uncompressed stream: None = every `block_bytes` bytes (records span block
boundaries freely), "record" = at every record boundary, or an explicit list; no block exceeds 65 280 bytes either way.
Returns dict(header_end, records=[dict(offset, fixed, name, cigar, seq, aux, end)]) - offsets of every part of every
record in the uncompressed stream, for tests that cut blocks inside a chosen field.
"""
import struct
import zlib

MAX_BLOCK = 0xFF00
_SEQ_TABLE = bytes.maketrans(b"=ACMGRSVTWYHKDBN", bytes(range(16)))
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def reg2bin(beg, end):
    """the UCSC bin of [beg, end) (specification 5.3)"""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _tag_bytes(tag):
    if len(tag) == 2:
        key, val = tag
        typ = "Z" if isinstance(val, str) else "f" if isinstance(val, float) else "i"
    else:
        key, typ, val = tag
    out = key.encode() + typ.encode()
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
    if typ == "A":
        return out + val.encode()
    if typ in fmt:
        return out + struct.pack(fmt[typ], val)
    if typ in ("Z", "H"):
        return out + val.encode() + b"\0"
    if typ == "B":
        sub, items = val
        return out + sub.encode() + struct.pack("<I", len(items)) + struct.pack("<%d%s" % (len(items), fmt[sub][1]), *items)
    raise ValueError("tag type %r" % typ)


def record_bytes(r, cg=False):
    """one alignment record, block_size included -> (bytes, offsets of its parts relative to the record's first byte)"""
    name = r["name"].encode() + b"\0"
    cigar = [(int(op), int(ln)) for op, ln in r["cigar"]]
    seq = r["seq"]
    l_seq = len(seq)
    ref_len = sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
    tags = [_tag_bytes(t) for t in r.get("tags", ())]
    if cg or len(cigar) > 65535:
        tags.append(_tag_bytes(("CG", "B", ("I", [ln << 4 | op for op, ln in cigar]))))
        cigar = [(4, l_seq), (3, ref_len)]
    start = int(r["start"])
    codes = seq.encode().translate(_SEQ_TABLE) + b"\0"                       # 4 bits per base, the first base in the high nibble
    packed = bytes(hi << 4 | lo for hi, lo in zip(codes[0:l_seq:2], codes[1 : l_seq + 1 : 2]))
    body = struct.pack("<iiBBHHHIiii", r.get("refid", 0), start, len(name), r["mapq"], reg2bin(max(start, 0), max(start, 0) + max(ref_len, 1)),
                       len(cigar), r["flag"], l_seq, -1, -1, 0)
    parts = [body, name, struct.pack("<%dI" % len(cigar), *[ln << 4 | op for op, ln in cigar]), packed, b"\xff" * l_seq, b"".join(tags)]
    offs, o = {}, 4
    for k, p in zip(("fixed", "name", "cigar", "seq", "qual", "aux"), parts):
        offs[k] = o
        o += len(p)
    offs["end"] = o
    blob = b"".join(parts)
    return struct.pack("<i", len(blob)) + blob, offs


def bgzf_block(data, level=6):
    assert len(data) <= MAX_BLOCK
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    bsize = 12 + 6 + len(comp) + 8 - 1
    assert bsize < 65536
    return (struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, bsize) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_bam(path, refs, records, sort_order="coordinate", cuts=None, block_bytes=MAX_BLOCK, cg=False, eof=True, level=6, truncate=0):
    text = ("@HD\tVN:1.6\tSO:%s\n" % sort_order + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in refs)).encode()
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, ln in refs:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    stream, info = [head], dict(header_end=len(head), records=[])
    o = len(head)
    for r in records:
        blob, offs = record_bytes(r, cg=cg)
        info["records"].append({k: v + o for k, v in offs.items()} | {"offset": o})
        stream.append(blob)
        o += len(blob)
    data = b"".join(stream)
    if cuts == "record":
        cuts = [info["header_end"]] + [x["offset"] for x in info["records"]]
    points = sorted(set(c for c in (cuts or ()) if 0 < c < len(data)))
    out, a = [], 0
    for b in points + [len(data)]:
        while a < b:                                      # no block above the limits, wherever the cuts are
            e = min(b, a + min(block_bytes, MAX_BLOCK))
            out.append(bgzf_block(data[a:e], level))
            a = e
    if eof:
        out.append(EOF_BLOCK)
    blob = b"".join(out)
    if truncate:
        blob = blob[: len(blob) - truncate]
    with open(path, "wb") as f:
        f.write(blob)
    info["n_blocks"] = len(out)
    return info
