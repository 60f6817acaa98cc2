"""An independent writer of bgzip's .gzi, for tests/test_bgzf_reference.py: it shares no code with cutesv_amd.fasta.

The format as `bgzip -i` writes it, restated from memory like the reader's (no bgzip is at hand to check either against; DESIGN.md
section 35 says so): a little-endian uint64 count, then that many pairs of uint64 - the compressed and the uncompressed offset at
which a block starts - for every block of the file but the first, whose pair (0, 0) is implied.  The end-of-file block is a block
like any other and has its entry.  What this writer is independent in is the walk: it goes over the gzip members of the
image by their own header fields (XLEN and the extra subfields, not a fixed layout) and takes each block's uncompressed size from
zlib, not from the trailer."""
import struct
import zlib


def members(image):
    """[(compressed offset, compressed size, uncompressed size)] of the gzip members of a BGZF image"""
    out, o = [], 0
    while o < len(image):
        magic, method, flags = struct.unpack_from("<HBB", image, o)
        assert magic == 0x8B1F and method == 8 and flags & 4, "no gzip member with an extra field at byte %d" % o
        xlen = struct.unpack_from("<H", image, o + 10)[0]
        sub, bsize = o + 12, None
        while sub < o + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", image, sub)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", image, sub + 4)[0]
            sub += 4 + slen
        assert bsize is not None, "the member at byte %d has no BC subfield" % o
        size = bsize + 1
        data = zlib.decompress(image[o + 12 + xlen:o + size - 8], -15)
        out.append((o, size, len(data)))
        o += size
    return out


def gzi_bytes(image):
    rows, u = [], 0
    for o, _, n in members(image):
        rows.append((o, u))
        u += n
    rows = rows[1:]
    return struct.pack("<Q", len(rows)) + b"".join(struct.pack("<QQ", c, v) for c, v in rows)
