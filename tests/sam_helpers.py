"""SAM text for the tests, and its judge.  Two independent pieces, neither of which imports the package under test:

    sam_line(record, refs)      one alignment line from the record dicts tests/bam_writer.py takes (plus optional qual, rnext, pnext, tlen)
    sam_text(refs, records)     a whole file: @HD, the @SQ lines, the alignment lines
    judge_record(line, ids)     one alignment line -> one BAM record, from SAMv1 sections 1.4, 1.5 and 4.2 with `struct` only; a float is
                                float(text) packed "<f"
    judge_stream(sam_bytes)     the whole inflated BAM stream a SAM file must give: header image and records

The conventions the specification leaves open are stated here as the project states them: bin = reg2bin(pos, pos + max(reference
length, 1)) & 0xffff with pos = POS - 1 (so POS 0 gives 4680), QUAL `*` = 0xff per base, an `i` value in the smallest of c C s S i I,
more than 65535 CIGAR operations as <l_seq>S<reference length>N plus a CG:B:I tag behind the line's own tags."""
import struct
import zlib

import bam_writer

BLOCK = 65280
_OPS = "MIDNSHP=X"
_BASES = "=ACMGRSVTWYHKDBN"
_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


# ------------------------------------------------------------------------------------------------ the writer
def _tag_text(tag):
    if len(tag) == 2:
        key, val = tag
        typ = "Z" if isinstance(val, str) else "f" if isinstance(val, float) else "i"
    else:
        key, typ, val = tag
    if typ in "cCsSiI":
        return "%s:i:%d" % (key, val)
    if typ == "f":
        return "%s:f:%s" % (key, val if isinstance(val, str) else repr(float(val)))
    if typ == "B":
        sub, items = val
        return "%s:B:%s%s" % (key, sub, "".join("," + (x if isinstance(x, str) else repr(float(x)) if sub == "f" else "%d" % x) for x in items))
    return "%s:%s:%s" % (key, typ, val)


def sam_line(r, refs):
    refid = r.get("refid", 0)
    cigar = "".join("%d%s" % (ln, _OPS[op]) for op, ln in r["cigar"]) or "*"
    fields = [r["name"], "%d" % r["flag"], "*" if refid < 0 else refs[refid][0], "%d" % (r["start"] + 1), "%d" % r["mapq"], cigar, r.get("rnext", "*"),
              "%d" % r.get("pnext", 0), "%d" % r.get("tlen", 0), r["seq"] or "*", r.get("qual", "*")]
    return "\t".join(fields + [_tag_text(t) for t in r.get("tags", ())])


def header_text(refs, sort_order="unsorted", hd=True, extra=""):
    return ("@HD\tVN:1.6\tSO:%s\n" % sort_order if hd else "") + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in refs) + extra


def sam_text(refs, records, **kw):
    return (header_text(refs, **kw) + "".join(sam_line(r, refs) + "\n" for r in records)).encode()


# ------------------------------------------------------------------------------------------------ the judge
def header_image(text, refs):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, ln in refs:
        out += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", ln)
    return out


def split_header(sam):
    """-> (header text bytes, [(name bytes, length)], body bytes)"""
    at, refs = 0, []
    while at < len(sam) and sam[at:at + 1] == b"@":
        e = sam.find(b"\n", at)
        e = len(sam) if e < 0 else e
        f = sam[at:e].split(b"\t")
        if f[0] == b"@SQ":
            d = {x[:2]: x[3:] for x in f[1:]}
            refs.append((d[b"SN"], int(d[b"LN"])))
        at = min(len(sam), e + 1)
    return sam[:at], refs, sam[at:]


def _int_tag(v):
    for typ, lo, hi in (("c", -128, -1), ("s", -32768, -1), ("i", -(1 << 31), -1)) if v < 0 else (("C", 0, 255), ("S", 0, 65535), ("I", 0, (1 << 32) - 1)):
        if lo <= v <= hi:
            return typ.encode() + struct.pack(_FMT[typ], v)
    raise ValueError("integer tag %d" % v)


def _tag(field):
    key, typ, val = field[:2], field[3:4], field[5:]
    assert field[2:3] == b":" and field[4:5] == b":"
    if typ == b"A":
        assert len(val) == 1
        return key + b"A" + val
    if typ == b"i":
        return key + _int_tag(int(val))
    if typ == b"f":
        return key + b"f" + struct.pack("<f", float(val))
    if typ in (b"Z", b"H"):
        return key + typ + val + b"\0"
    if typ == b"B":
        sub = val[:1].decode()
        items = val[2:].split(b",") if len(val) > 1 else []
        conv = float if sub == "f" else int
        return key + b"B" + sub.encode() + struct.pack("<I", len(items)) + b"".join(struct.pack(_FMT[sub], conv(x)) for x in items)
    raise ValueError("tag type %r" % typ)


def judge_record(line, ids):
    """line: bytes without the line break; ids: {name bytes: refid}"""
    f = line.split(b"\t")
    assert len(f) >= 11
    name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    refid = -1 if rname == b"*" else ids[rname]
    next_refid = -1 if rnext == b"*" else refid if rnext == b"=" else ids[rnext]
    ops, num = [], 0
    if cigar != b"*":
        for c in cigar.decode():
            if c.isdigit():
                num = num * 10 + int(c)
            else:
                ops.append((num << 4) | _OPS.index(c))
                num = 0
    ref_len = sum(w >> 4 for w in ops if (w & 15) in (0, 2, 3, 7, 8))
    l_seq = 0 if seq == b"*" else len(seq)
    codes = [(_BASES.index(c) if c in _BASES else 15) for c in seq.decode().upper()] if l_seq else []
    codes.append(0)
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
    quals = b"\xff" * l_seq if qual == b"*" else bytes(q - 33 for q in qual)
    assert len(quals) == l_seq
    tags = b"".join(_tag(x) for x in f[11:])
    words = ops
    if len(ops) > 65535:
        tags += b"CGBI" + struct.pack("<I", len(ops)) + struct.pack("<%dI" % len(ops), *ops)
        words = [l_seq << 4 | 4, ref_len << 4 | 3]
    p = int(pos) - 1
    body = struct.pack("<iiBBHHHIiii", refid, p, len(name) + 1, int(mapq), bam_writer.reg2bin(p, p + max(ref_len, 1)) & 0xFFFF, len(words), int(flag), l_seq, next_refid,
                       int(pnext) - 1, int(tlen))
    blob = body + name + b"\0" + struct.pack("<%dI" % len(words), *words) + packed + quals + tags
    return struct.pack("<i", len(blob)) + blob


def judge_stream(sam):
    text, refs, body = split_header(sam)
    ids = {n: i for i, (n, _) in enumerate(refs)}
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return header_image(text, refs) + b"".join(judge_record(ln, ids) for ln in lines)


# ------------------------------------------------------------------------------------------------ files
def blocks_of(blob):
    """[(offset, block size, isize)] of a BGZF file"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 14] == b"BC"
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        out.append((at, size, struct.unpack_from("<I", blob, at + size - 4)[0]))
        at += size
    assert at == len(blob)
    return out


def inflate_file(path):
    with open(path, "rb") as f:
        blob = f.read()
    out = []
    for at, size, isize in blocks_of(blob):
        data = zlib.decompress(blob[at + 18:at + size - 8], -15)
        assert len(data) == isize and zlib.crc32(data) & 0xFFFFFFFF == struct.unpack_from("<I", blob, at + size - 8)[0]
        out.append(data)
    return b"".join(out)


def check_file(blob, want):
    blocks = blocks_of(blob)
    assert blob[-28:] == bam_writer.EOF_BLOCK and blocks[-1][2] == 0
    assert [isize for _, _, isize in blocks[:-1]] == [min(BLOCK, len(want) - a) for a in range(0, len(want), BLOCK)]
    return blocks


def tiny(name, refid, start, flag=0, seq="ACGT", cigar=None, **kw):
    return dict(name=name, flag=flag, mapq=60, start=start, refid=refid, cigar=[(0, len(seq))] if cigar is None else cigar, seq=seq, **kw)
