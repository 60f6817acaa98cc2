"""An independent writer of tabix indexes (.tbi) for VCF text, from the format's description (the tabix format note and SAMv1
section 5.2 for bins and the linear index): the test-side twin of cutesv_amd.bgzf.tabix_vcf.  It shares no code with
cutesv_amd/csrc/index_core.h: dictionaries and lists, one record at a time.

    tbi_bytes(text, block_table) -> the bytes of the .tbi before its BGZF compression
    voff(block_table, u)         -> the virtual offset of stream byte u
    seek_line(image, v)          -> the line that starts at virtual offset v of a BGZF file image

Layout: "TBI\\1", n_ref, format (2: VCF), col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm, the NUL-terminated names; then per
name n_bin, {bin, n_chunk, {beg, end}}, n_intv, {ioff}; then n_no_coor.  Bins ascending, the pseudo-bin 37450 last with the
{first record's start, last record's end} and {records, 0} pairs; a chunk is a maximal stretch of neighbouring lines in one bin; an
empty 16 kb window takes the offset of the next window that has one.  Names are numbered in order of first appearance."""
import bisect
import struct
import zlib

PSEUDO_BIN = 37450
MAX_POS = 1 << 29


class Refused(ValueError):
    pass


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def voff(table, u):
    """byte u of the stream lies in the block that holds it; a byte on a block boundary - and the end of the stream - belongs to the
    next block that is not empty, or to the last block (the end-of-file block), at offset 0"""
    uoff, coff, isize = ([int(x) for x in col] for col in table)
    k = bisect.bisect_right(uoff, u) - 1
    while k + 1 < len(uoff) and isize[k] == 0:
        k += 1
    assert 0 <= u - uoff[k] < 65536
    return coff[k] << 16 | (u - uoff[k])


def interval(line):
    """(name, beg, end) of a VCF data line: beg = POS - 1; end = INFO's END= value when greater than beg, else beg + len(REF)"""
    col = line.rstrip(b"\n").split(b"\t")
    name, beg = col[0], int(col[1]) - 1
    end = beg + len(col[3])
    if len(col) > 7:
        for item in col[7].split(b";"):
            if item.startswith(b"END="):
                digits = item[4:]
                if digits.isdigit() and int(digits) > beg:
                    end = int(digits)
                break
    return name, beg, end


def tbi_bytes(text, table):
    names, refs = [], []                                   # per name: dict(bins={bin: [[beg, end], ...]}, lin={window: offset}, first, last, n)
    u, ordinal, prev = 0, 0, None                          # prev: (ref id, beg, bin) of the line before
    for line in text.splitlines(keepends=True):
        u0, u = u, u + len(line)
        if line.startswith(b"#") or line == b"\n":
            continue
        name, beg, end = interval(line)
        beg_c, end_c = max(beg, 0), max(end, max(beg, 0) + 1)
        if beg + 1 >= MAX_POS or end_c > MAX_POS:                # a POS at or beyond 2^29, or an end beyond it
            raise Refused("line %d reaches 2^29" % ordinal)
        if name not in names:
            names.append(name)
            refs.append(dict(bins={}, lin={}, first=None, last=None, n=0))
        rid = names.index(name)
        if prev is not None and (rid < prev[0] or (rid == prev[0] and beg < prev[1])):
            raise Refused("line %d is out of order" % ordinal)
        b = reg2bin(beg_c, end_c)
        v0, v1 = voff(table, u0), voff(table, u)
        R = refs[rid]
        if prev is not None and prev[0] == rid and prev[2] == b:
            R["bins"][b][-1][1] = v1
        else:
            R["bins"].setdefault(b, []).append([v0, v1])
        for w in range(beg_c >> 14, ((end_c - 1) >> 14) + 1):
            R["lin"][w] = min(R["lin"].get(w, v0), v0)
        if R["first"] is None:
            R["first"] = v0
        R["last"] = v1
        R["n"] += 1
        prev = (rid, beg, b)
        ordinal += 1
    o = [b"TBI\x01", struct.pack("<8i", len(names), 2, 1, 2, 0, ord("#"), 0, sum(len(n) + 1 for n in names))]
    o += [n + b"\x00" for n in names]
    for R in refs:
        o.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            o.append(struct.pack("<Ii", b, len(R["bins"][b])))
            o += [struct.pack("<QQ", c0, c1) for c0, c1 in R["bins"][b]]
        o.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["first"], R["last"], R["n"], 0))
        n_intv = max(R["lin"]) + 1
        lin, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            nxt = R["lin"].get(w, nxt)
            lin[w] = nxt
        o.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *lin))
    o.append(struct.pack("<Q", 0))
    return b"".join(o)


def chunk_offsets(tbi):
    """every virtual offset that starts a chunk or fills a linear-index entry of an (uncompressed) .tbi, the pseudo-bin's first pair included"""
    n_ref, l_nm = struct.unpack_from("<i", tbi, 4)[0], struct.unpack_from("<i", tbi, 32)[0]
    p, out = 36 + l_nm, set()
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", tbi, p); p += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", tbi, p); p += 8
            for c in range(n_chunk):
                if b != PSEUDO_BIN or c == 0:
                    out.add(struct.unpack_from("<Q", tbi, p)[0])
                p += 16
        (n_intv,) = struct.unpack_from("<i", tbi, p); p += 4
        out.update(struct.unpack_from("<%dQ" % n_intv, tbi, p)); p += 8 * n_intv
    assert p + 8 == len(tbi)
    return sorted(out)


def seek_line(image, v):
    """the bytes from virtual offset v up to and including the next newline: the block at v >> 16 is inflated, and the one behind it
    when the line goes on there"""
    coff, uoff = v >> 16, v & 0xFFFF
    out = b""
    while b"\n" not in out[uoff:]:
        size = struct.unpack_from("<H", image, coff + 16)[0] + 1
        out += zlib.decompress(image[coff + 18 : coff + size - 8], -15)
        coff += size
        if coff >= len(image):
            break
    return out[uoff : out.index(b"\n", uoff) + 1]
