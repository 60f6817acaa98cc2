"""The BGZF writer and the tabix index: out.vcf.gz and out.vcf.gz.tbi without bgzip and tabix.

    compress(data, ctx=None, route=None)   -> (the file image, ending in the end-of-file block; the block table)
    tabix_vcf(text, block_table)           -> the bytes of the .tbi (itself BGZF-compressed)
    compress_kept(ctx, kept)               -> the same pair for a text a device emit left on the context
    tabix_rows(kept, block_table)          -> the .tbi of that text from the emitter's rows: the text never comes down
    python -m cutesv_amd.bgzf FILE [-o OUT] [--tabix] [--route host|device]

The input is cut every 65280 bytes, bgzip's cut: the stored form of such a block is 65311 bytes, so a block that does not compress
still fits the format's 65536.  Routes:
    "device"   csv_bgzf_deflate: one wavefront per block (cutesv_amd/csrc/deflate_core.h, k_bgzf_deflate at the end of bam.hip.h)
    "host"     zlib.compressobj(6, zlib.DEFLATED, -15) per block on a small thread pool: what bgzip gives, and the timing baseline
    "core"     csv_bgzf_deflate_host: the device's core with one lane on one host thread - byte for byte the device's image; for checks
The routes differ in the compressed bytes, never in what they inflate to.

The block table is (uoff, coff, isize), one row per block with the end-of-file block last: the shape index_core.h's IxBlocks
takes, so a byte of the text has the virtual offset ix_voff gives it.  tabix_vcf hands text and table to csv_tbx_build
(cutesv_amd/csrc/bgzf_host.cpp), which holds the interval rule in one function: beg = POS - 1, end = INFO's END= when that is greater
than beg, else beg + len(REF).  The rule restates htslib's from memory; it has not been checked against tabix itself."""
import argparse
import ctypes as C
import struct
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._lib import lib

BLOCK = 65280                           # input bytes per BGZF block (bgzip's 0xff00)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
ROUTES = ("host", "device", "core")
DEFAULT_ROUTE = "host"                  # the rule of section 34: "device" only if its wall is below the host route's on both measured inputs
HOST_THREADS = 4
_HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")


class BgzfError(RuntimeError):
    pass


def _cuts(n):
    """-> (offsets int64[k], lengths int32[k]) of the pieces of n bytes"""
    off = np.arange(0, n, BLOCK, dtype=np.int64)
    ln = np.minimum(BLOCK, n - off).astype(np.int32)
    return off, ln


def _host_block(piece, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(piece) + co.flush()
    return b"".join((_HEAD, struct.pack("<H", len(payload) + 25), payload, struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece))))


def deflate_blocks(ctx, data, in_off, in_len, route="device", cap=None, guard=0, coding=False):
    """csv_bgzf_deflate ("device") or csv_bgzf_deflate_host ("core") on the pieces data[in_off[k] : in_off[k] + in_len[k]] ->
    (image uint8[out_bytes] - empty when out_bytes exceeds cap -, block_bytes int32[n], out_bytes, ms_kernels).  cap: the capacity handed
    to the call (default: the bound, every block stored); guard: that many bytes of 0xA5 stand behind the capacity and are returned as
    a fifth item; coding ("core" only): a sixth item, int32[n, 3] - the payload bytes of the stored, fixed and dynamic coding."""
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    in_off, in_len = np.ascontiguousarray(in_off, np.int64), np.ascontiguousarray(in_len, np.int32)
    n = len(in_len)
    if cap is None:
        cap = int(in_len.sum(dtype=np.int64)) + 31 * n
    out = np.full(cap + guard, 0xA5, np.uint8) if guard else np.empty(cap, np.uint8)
    sizes = np.zeros(n, np.int32)
    need, ms = C.c_int64(-1), C.c_double(0)
    cod = np.zeros((n, 3), np.int32)
    ptr = lambda a: a.ctypes.data if len(a) else None                              # noqa: E731
    if route == "device":
        rc = lib().csv_bgzf_deflate(ctx._h, ptr(buf), len(buf), n, ptr(in_off), ptr(in_len), ptr(out), cap, ptr(sizes), C.byref(need), 0, C.byref(ms))
        ctx._check(rc)
    else:
        rc = lib().csv_bgzf_deflate_host(ptr(buf), len(buf), n, ptr(in_off), ptr(in_len), ptr(out), cap, ptr(sizes), C.byref(need), ptr(cod))
        if rc:
            raise BgzfError("csv_bgzf_deflate_host refused the call (%d)" % rc)
    image = out[: need.value] if need.value <= cap else out[:0]
    res = [image, sizes, int(need.value), float(ms.value)]
    if guard or coding:
        res.append(out[cap:])
    if coding:
        res.append(cod)
    return tuple(res)


def compress(data, ctx=None, route=None, level=6, threads=HOST_THREADS, timings=None):
    """data (bytes-like) -> (image bytes, (uoff int64[n + 1], coff int64[n + 1], isize uint32[n + 1])): BGZF blocks of at most 65280
    input bytes each and the end-of-file block, whose row is the table's last.  route: None (DEFAULT_ROUTE), "host" (zlib at `level` on
    `threads` threads), "device" (ctx: an engine.Context; None: one is opened on device 0 for the call) or "core"."""
    route = DEFAULT_ROUTE if route is None else route
    if route not in ROUTES:
        raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
    view = memoryview(data).cast("B") if not isinstance(data, (bytes, bytearray)) else data
    n = len(view)
    off, ln = _cuts(n)
    if route == "host":
        pieces = [view[int(o) : int(o) + int(k)] for o, k in zip(off, ln)]
        if threads > 1 and len(pieces) > 1:
            with ThreadPoolExecutor(threads) as pool:
                blocks = list(pool.map(lambda p: _host_block(p, level), pieces))
        else:
            blocks = [_host_block(p, level) for p in pieces]
        sizes = np.array([len(b) for b in blocks], np.int64)
        image = b"".join(blocks) + EOF_BLOCK
    else:
        own = None
        if route == "device" and ctx is None:
            from . import engine
            own = ctx = engine.Context(0)
        try:
            img, sizes, need, ms = deflate_blocks(ctx, view, off, ln, route=route)[:4]
        finally:
            if own is not None:
                own.close()
        if timings is not None:
            timings["ms_bgzf_kernels"] = ms
        sizes = sizes.astype(np.int64)
        image = img.tobytes() + EOF_BLOCK
    coff = np.zeros(len(off) + 1, np.int64)
    coff[1:] = np.cumsum(sizes)
    uoff = np.append(off, np.int64(n))
    isize = np.append(ln.astype(np.uint32), np.uint32(0))
    return image, (uoff, coff, isize)


def compress_kept(ctx, kept, timings=None):
    """csv_bgzf_deflate_text: the text a device emit left on `ctx` (kept: a vcf.KeptText) compressed where it lies -> (image bytes, block
    table), as compress gives them for the same bytes on route "device"; only the compressed blocks come down"""
    kept.check()
    n = kept.n_bytes
    off, ln = _cuts(n)
    nb = len(ln)
    cap = n + 31 * nb
    out, sizes = np.empty(max(cap, 1), np.uint8), np.zeros(max(nb, 1), np.int32)
    need, ms = C.c_int64(-1), C.c_double(0)
    ptr = lambda a: a.ctypes.data if len(a) else None                              # noqa: E731
    ctx._check(lib().csv_bgzf_deflate_text(ctx._h, nb, ptr(off), ptr(ln), out.ctypes.data, cap, sizes.ctypes.data, C.byref(need), C.byref(ms)))
    if timings is not None:
        timings["ms_bgzf_kernels"] = ms.value
    coff = np.zeros(nb + 1, np.int64)
    coff[1:] = np.cumsum(sizes[:nb].astype(np.int64))
    return out[: need.value].tobytes() + EOF_BLOCK, (np.append(off, np.int64(n)), coff, np.append(ln.astype(np.uint32), np.uint32(0)))


def tabix_rows_raw(names, rows, text_bytes, block_table):
    """csv_tbx_build_rows: the .tbi of the records `rows` describes (int64[n, 4]: name index, beg, end, offset) in a text of text_bytes
    bytes that lies in the blocks of `block_table`, before its own compression - the bytes csv_tbx_build gives over that text"""
    uoff, coff, isize = (np.ascontiguousarray(a, dt) for a, dt in zip(block_table, (np.int64, np.int64, np.uint32)))
    if not (len(uoff) == len(coff) == len(isize) >= 1):
        raise ValueError("the block table needs one row per block, the end-of-file block included")
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 4)
    enc = [s.encode() for s in names]
    blob = b"".join(enc)
    noff = np.zeros(len(enc) + 1, np.int64)
    if enc:
        noff[1:] = np.cumsum([len(e) for e in enc])
    need, err = C.c_int64(0), C.create_string_buffer(512)
    out = np.zeros(1 << 16, np.uint8)
    for _ in range(2):
        rc = lib().csv_tbx_build_rows(blob, noff.ctypes.data, len(enc), rows.ctypes.data if len(rows) else None, len(rows), int(text_bytes), len(uoff), uoff.ctypes.data,
                                      coff.ctypes.data, isize.ctypes.data, out.ctypes.data, len(out), C.byref(need), err, len(err))
        if rc:
            raise BgzfError(err.value.decode() or "csv_tbx_build_rows failed (%d)" % rc)
        if need.value <= len(out):
            return out[: need.value].tobytes()
        out = np.zeros(need.value, np.uint8)
    raise BgzfError("csv_tbx_build_rows: the size changed between two calls")


def tabix_rows(kept, block_table, ctx=None, route="host"):
    """-> the bytes of out.vcf.gz.tbi for a kept text (vcf.KeptText) whose compressed blocks `block_table` describes (compress_kept's second
    result): tabix_vcf's bytes, from the rows the emitter wrote beside the text instead of the text"""
    return compress(tabix_rows_raw(kept.names, kept.rows, kept.n_bytes, block_table), ctx=ctx, route=route)[0]


def blocks_of(image):
    """the BGZF blocks of a file image -> [(offset, size, isize)]; raises BgzfError on anything that is no BGZF block"""
    out, o = [], 0
    while o < len(image):
        if len(image) - o < 28 or bytes(image[o : o + 4]) != b"\x1f\x8b\x08\x04" or bytes(image[o + 10 : o + 16]) != b"\x06\x00BC\x02\x00":
            raise BgzfError("no BGZF block at byte %d" % o)
        size = struct.unpack_from("<H", image, o + 16)[0] + 1
        if size < 26 or o + size > len(image):
            raise BgzfError("the BGZF block at byte %d is cut short" % o)
        out.append((o, size, struct.unpack_from("<I", image, o + size - 4)[0]))
        o += size
    return out


def decompress(image):
    """the text of a BGZF file image (zlib per block, CRC32 and ISIZE checked)"""
    parts = []
    for o, size, isize in blocks_of(image):
        d = zlib.decompress(bytes(image[o + 18 : o + size - 8]), -15)
        if len(d) != isize or (zlib.crc32(d) & 0xFFFFFFFF) != struct.unpack_from("<I", image, o + size - 8)[0]:
            raise BgzfError("the BGZF block at byte %d fails its CRC32 or ISIZE" % o)
        parts.append(d)
    return b"".join(parts)


def tabix_raw(text, block_table):
    """csv_tbx_build: the .tbi of VCF `text` (bytes) that lies in the blocks of `block_table`, before its own compression"""
    uoff, coff, isize = (np.ascontiguousarray(a, dt) for a, dt in zip(block_table, (np.int64, np.int64, np.uint32)))
    if not (len(uoff) == len(coff) == len(isize) >= 1):
        raise ValueError("the block table needs one row per block, the end-of-file block included")
    buf = np.frombuffer(text, np.uint8)
    need, err = C.c_int64(0), C.create_string_buffer(512)
    out = np.zeros(1 << 16, np.uint8)
    for _ in range(2):
        rc = lib().csv_tbx_build(buf.ctypes.data if len(buf) else None, len(buf), len(uoff), uoff.ctypes.data, coff.ctypes.data, isize.ctypes.data,
                                 out.ctypes.data, len(out), C.byref(need), err, len(err))
        if rc:
            raise BgzfError(err.value.decode() or "csv_tbx_build failed (%d)" % rc)
        if need.value <= len(out):
            return out[: need.value].tobytes()
        out = np.zeros(need.value, np.uint8)
    raise BgzfError("csv_tbx_build: the size changed between two calls")


def tabix_vcf(text, block_table, ctx=None, route="host"):
    """-> the bytes of out.vcf.gz.tbi for the VCF `text` whose compressed blocks `block_table` describes (compress's second result)"""
    return compress(tabix_raw(text, block_table), ctx=ctx, route=route)[0]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cutesv_amd.bgzf", description="BGZF-compress FILE (and index it as VCF with --tabix)")
    ap.add_argument("file")
    ap.add_argument("-o", "--output", default=None, help="the compressed file [FILE.gz]")
    ap.add_argument("--tabix", action="store_true", help="also write OUTPUT.tbi: FILE is VCF text")
    ap.add_argument("--route", default=None, choices=["host", "device"], help="[%s]" % DEFAULT_ROUTE)
    a = ap.parse_args(argv)
    out = a.output or a.file + ".gz"
    with open(a.file, "rb") as f:
        text = f.read()
    ctx = None
    if a.route == "device" or (a.route is None and DEFAULT_ROUTE == "device"):
        from . import engine
        ctx = engine.Context(0)
    try:
        image, table = compress(text, ctx=ctx, route=a.route)
        tbi = tabix_vcf(text, table) if a.tabix else None
    finally:
        if ctx is not None:
            ctx.close()
    with open(out, "wb") as f:
        f.write(image)
    if tbi is not None:
        with open(out + ".tbi", "wb") as f:
            f.write(tbi)
    print("cutesv_amd.bgzf: %d bytes -> %d bytes in %d blocks%s" % (len(text), len(image), len(table[0]), ", index in %s.tbi" % out if a.tabix else ""), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
