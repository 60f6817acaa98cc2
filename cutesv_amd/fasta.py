"""The reference genome for the VCF emit step, without pysam (cuteSV_genotype.py:254-259: generate_output opens
`pysam.FastaFile(ref)` and fetches whole chromosomes).

`Reference(path)` maps the FASTA file into memory (mmap: nothing is read until a base is looked at, nothing is copied into
Python strings - a human reference is 3.1 GB) and indexes it like `samtools faidx`: from `<path>.fai` when it sits next to
the file, else with one pass of the native indexer (`csv_fasta_index`, cutesv_amd/csrc/vcf_emit.cpp).  `csv_vcf_emit` then
reads REF / ALT bases straight out of the mapping through (line_bases, line_width) arithmetic (include/cutesv_hip.h
csv_vcf_in.chrom_line_bases).

A BGZF-compressed FASTA (`ref.fa.gz` from bgzip, with its `.fai` and `.gzi` beside it or without) cannot be mapped; it is never
inflated whole either.  `open_reference(path)` looks at the content and gives a `Reference` for plain text
and a `BgzfReference` for BGZF.  `BgzfReference.gather` inflates only the blocks the asked base ranges touch and cuts the ranges out
of them: on the host ("host": zlib on a few threads, then ref_core.h's host form) or on the device ("device": csv_ref_gather, the
blocks inflated by k_bgzf_inflate and cut by k_ref_gather without leaving device memory).  A `.fai` that is missing is built window
by window through csv_fasta_index_stream (on the "device" route from the event rows of k_fai_events, which finds the lines on the device); a `.gzi` that is missing is built by hopping over the block headers, with no inflate.
A plain gzip file has no blocks to address: it is refused, and `read_fasta` (whole contigs as str, round 1's reader) remains for it
and for tests.

    python -m cutesv_amd.fasta FILE --faidx [--route host|device] [--write]      the .fai (and the .gzi) of a FASTA file, plain or BGZF
"""
import argparse
import contextlib
import ctypes as C
import gzip
import mmap
import os
import struct
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _abi
from ._lib import lib

REF_ROUTES = ("host", "device")
DEFAULT_REF_ROUTE = "host"              # DESIGN.md section 35 has the measurement and why the default did not move with it
WINDOW_BLOCKS = 4096                    # CSV_BAM_WINDOW_BLOCKS (include/cutesv_hip.h): touched blocks per gather call
HOST_THREADS = 4                        # zlib threads of the host route when the caller names none (the command lines pass -t / --threads)
FAI_ROW_CAP = 1 << 16                   # event rows a window may bring down on the device route of the .fai build (24 bytes each) ...
FAI_HDR_CAP = 1 << 20                   # ... and the bytes of its header texts; a window beyond either is indexed by the host form


def _parse_fai(fai, path, size):
    """the rows of a .fai whose offsets must lie inside `size` bytes -> (names, length, offset, line_bases, line_width)"""
    names, rows = [], []
    with open(fai) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) < 5:
                continue
            names.append(p[0])
            rows.append([int(x) for x in p[1:5]])
    t = np.array(rows, np.int64).reshape(-1, 4)
    length, offset = t[:, 0].copy(), t[:, 1].copy()
    line_bases, line_width = t[:, 2].astype(np.int32), t[:, 3].astype(np.int32)
    # a stale or foreign index must not send the emitter past the mapping
    last = offset + np.where(line_bases > 0, (np.maximum(length, 1) - 1) // np.maximum(line_bases, 1) * line_width
                             + (np.maximum(length, 1) - 1) % np.maximum(line_bases, 1), 0)
    # (a contig without sequence - a header at the end of the file, length 0: samtools writes the same entry - has nothing to
    # read: its offset may equal the file size)
    has = length > 0
    if len(t) and ((has.any() and int(last[has].max()) >= size) or int(offset.min()) < 0 or int(offset.max()) > size):
        raise ValueError("%s does not describe %s (offsets beyond the file)" % (fai, path))
    return names, length, offset, line_bases, line_width


class Reference:
    """contig name -> (offset, length, line_bases, line_width) over a memory-mapped FASTA file"""

    def __init__(self, path, fai=None, write_fai=False):
        self.path = str(path)
        if self.path.endswith(".gz"):
            raise ValueError("a gzip-compressed FASTA cannot be memory-mapped: decompress it (or bgzip + faidx upstream), or use fasta.read_fasta")
        self._f = open(self.path, "rb")
        self.size = os.fstat(self._f.fileno()).st_size
        self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ) if self.size else None
        self._buf = np.frombuffer(self._mm, np.uint8) if self._mm is not None else np.zeros(0, np.uint8)
        self.base_addr = int(self._buf.ctypes.data) if self.size else 0
        fai = fai or self.path + ".fai"
        if os.path.exists(fai) and os.path.getmtime(fai) >= os.path.getmtime(self.path):
            self._read_fai(fai)
        else:
            self._build()
            if write_fai:
                self.write_fai(fai)
        self.index = {n: i for i, n in enumerate(self.names)}

    # ---- index
    def _read_fai(self, fai):
        self.names, self.length, self.offset, self.line_bases, self.line_width = _parse_fai(fai, self.path, self.size)

    def _build(self):
        cap = 1024
        while True:
            name_off, name_len = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
            length, offset = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
            lb, lw = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            n = lib().csv_fasta_index(C.c_void_p(self.base_addr), self.size, cap, name_off.ctypes.data, name_len.ctypes.data,
                                      length.ctypes.data, offset.ctypes.data, lb.ctypes.data, lw.ctypes.data)
            if n < 0:
                raise ValueError("%s cannot be indexed (sequence before a header, or lines of unequal length inside a contig)" % self.path)
            if n <= cap:
                break
            cap = int(n)
        self.names = [bytes(self._buf[int(name_off[i]):int(name_off[i]) + int(name_len[i])]).decode() for i in range(n)]
        self.length, self.offset, self.line_bases, self.line_width = length[:n], offset[:n], lb[:n], lw[:n]

    def write_fai(self, fai=None):
        with open(fai or self.path + ".fai", "w") as f:
            for i, nm in enumerate(self.names):
                f.write("%s\t%d\t%d\t%d\t%d\n" % (nm, self.length[i], self.offset[i], self.line_bases[i], self.line_width[i]))

    # ---- access
    def __contains__(self, name):
        return name in self.index

    def contig(self, name):
        """(address of the first base, length, line_bases, line_width) - what csv_vcf_in takes per chromosome"""
        i = self.index[name]
        return self.base_addr + int(self.offset[i]), int(self.length[i]), int(self.line_bases[i]), int(self.line_width[i])

    def fetch(self, name, start=0, end=None):
        """bases [start, end) of a contig as str (pysam.FastaFile.fetch); for tests and small slices"""
        i = self.index[name]
        n, lb, lw, off = int(self.length[i]), int(self.line_bases[i]), int(self.line_width[i]), int(self.offset[i])
        end = n if end is None else min(end, n)
        start = max(0, start)
        if end <= start:
            return ""
        lo = off + (start // lb) * lw + start % lb
        hi = off + ((end - 1) // lb) * lw + (end - 1) % lb + 1
        raw = bytes(self._buf[lo:hi])
        return raw.replace(b"\r", b"").replace(b"\n", b"").decode()

    def close(self):
        self._buf = None
        if self._mm is not None:
            try:
                self._mm.close()
            except BufferError:          # (numpy views still alive: released with them)
                pass
        self._f.close()


# ------------------------------------------------------------------------------------ BGZF
class BgzfReferenceError(ValueError):
    pass


def _is_bgzf_header(b):
    """is b (at least 18 bytes) the head of a BGZF block: gzip magic, deflate, FEXTRA, and a `BC` subfield of two bytes"""
    if len(b) < 18 or bytes(b[:3]) != b"\x1f\x8b\x08" or not (b[3] & 4):
        return False
    xlen = b[10] | (b[11] << 8)
    ext, o = bytes(b[12:12 + xlen]), 0
    while o + 4 <= len(ext):
        slen = ext[o + 2] | (ext[o + 3] << 8)
        if ext[o:o + 2] == b"BC" and slen == 2:
            return True
        o += 4 + slen
    return False


def sniff(path):
    """-> "text", "bgzf" or "gzip", by content: the name says nothing"""
    try:
        with open(path, "rb") as f:
            head = f.read(1024)
    except OSError:                         # (a file that cannot be read is Reference's to report, as before)
        return "text"
    if head[:2] != b"\x1f\x8b":
        return "text"
    return "bgzf" if _is_bgzf_header(head) else "gzip"


def open_reference(path, ctx=None, route=None, threads=None, **kw):
    """the reference for the emit step, as pysam.FastaFile takes it: a `Reference` for plain text, a `BgzfReference` for a
    BGZF-compressed file (bgzip's output, whatever its name); a plain gzip file is refused.  ctx / route: the context and the route
    of BgzfReference.gather ("host", "device"; None: DEFAULT_REF_ROUTE) and the zlib threads of its host route (None: HOST_THREADS; the
    command lines pass their -t / --threads) - a plain-text reference has no use for them."""
    kind = sniff(path)
    if kind == "gzip":
        raise BgzfReferenceError("%s is gzip-compressed but has no BGZF blocks: a compressed reference must be compressed with bgzip "
                                 "(bgzip's blocks are what makes it addressable), or be given as plain text" % path)
    if kind == "bgzf":
        return BgzfReference(path, ctx=ctx, route=route, threads=HOST_THREADS if threads is None else threads, **kw)
    if route is not None and route not in REF_ROUTES:
        raise ValueError("route must be one of %s, not %r" % (", ".join(REF_ROUTES), route))
    return Reference(path, **kw)


@contextlib.contextmanager
def opened_reference(path, threads=None):
    """open_reference for a command line: the mapping, the descriptor and the thread pool are released at the end, whatever the call did"""
    reference = open_reference(path, threads=threads)
    try:
        yield reference
    finally:
        if hasattr(reference, "close"):         # (both kinds have it; a stand-in without one is left alone)
            reference.close()


def parse_gzi(data, what=".gzi"):
    """the bytes of a .gzi -> (coff int64[n], uoff int64[n]): where every block but the first starts, compressed and uncompressed.
    The format - a little-endian u64 count, then that many (compressed offset, uncompressed offset) u64 pairs - restates bgzip's
    from memory."""
    if len(data) < 8:
        raise BgzfReferenceError("%s is cut short: it has no entry count" % what)
    n = struct.unpack_from("<Q", data, 0)[0]
    if len(data) != 8 + 16 * n:
        raise BgzfReferenceError("%s says %d entries and holds %d bytes, not %d" % (what, n, len(data), 8 + 16 * n))
    t = np.frombuffer(data, "<u8", 2 * n, 8).reshape(n, 2)
    if n and int(t.max()) >= 1 << 62:          # (what int64 cannot hold; whether the offsets lie inside the file is _set_table's to say)
        raise BgzfReferenceError("%s holds an offset of 2^62 or more" % what)
    return t[:, 0].astype(np.int64), t[:, 1].astype(np.int64)


def gzi_bytes(coff, uoff):
    """the .gzi of the block table (coff, uoff: every block's start, the first block's (0, 0) included)"""
    t = np.empty((max(len(coff) - 1, 0), 2), "<u8")
    t[:, 0], t[:, 1] = coff[1:], uoff[1:]
    return struct.pack("<Q", len(t)) + t.tobytes()


class BgzfReference:
    """contig name -> bases of a BGZF-compressed FASTA, through its `.fai` (offsets in uncompressed coordinates) and its block table
    (`.gzi`).  names / length / __contains__ / fetch / close as Reference; gather: many ranges at once, on either route.

    path + ".gzi" and path + ".fai" are read when they exist and are not older than the file; a missing one is built in memory
    (written beside the file with write_gzi / write_fai).  stats: windows gathered per route, blocks read, windows the host served
    after the device reported a block."""

    def __init__(self, path, fai=None, gzi=None, write_fai=False, write_gzi=False, ctx=None, route=None, threads=HOST_THREADS, window_blocks=WINDOW_BLOCKS,
                 fai_row_cap=FAI_ROW_CAP, fai_hdr_cap=FAI_HDR_CAP):
        if route is not None and route not in REF_ROUTES:
            raise ValueError("route must be one of %s, not %r" % (", ".join(REF_ROUTES), route))
        self.path, self.ctx, self.route, self.threads, self.window_blocks = str(path), ctx, route, max(1, int(threads)), max(1, int(window_blocks))
        self.fai_row_cap, self.fai_hdr_cap = max(0, int(fai_row_cap)), max(0, int(fai_hdr_cap))
        self._pool = None
        self._f = open(self.path, "rb")
        self._mm = None
        try:
            self.csize = os.fstat(self._f.fileno()).st_size
            self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ) if self.csize else None
            self.stats = dict(windows_host=0, windows_device=0, blocks=0, windows_host_after_device=0, fai_windows_host=0, fai_windows_device=0, fai_windows_overflow=0,
                              fai_windows_host_after_device=0, fai_rows=0, ms_fai_inflate=0.0, ms_fai_events=0.0)
            if self.csize < 28 or not _is_bgzf_header(self._mm[:1024]):
                raise BgzfReferenceError("%s does not start with a BGZF block: a compressed reference must be compressed with bgzip" % self.path)
            gzi = gzi or self.path + ".gzi"
            if os.path.exists(gzi) and os.path.getmtime(gzi) >= os.path.getmtime(self.path):
                with open(gzi, "rb") as f:
                    coff, uoff = parse_gzi(f.read(), gzi)
                self._set_table(np.concatenate([[0], coff]).astype(np.int64), np.concatenate([[0], uoff]).astype(np.int64), gzi)
                self.gzi_built = False
            else:
                self._set_table(np.zeros(1, np.int64), np.zeros(1, np.int64), None)
                self.gzi_built = True
                if write_gzi:
                    self.write_gzi(gzi)
            fai = fai or self.path + ".fai"
            if os.path.exists(fai) and os.path.getmtime(fai) >= os.path.getmtime(self.path):
                self.names, self.length, self.offset, self.line_bases, self.line_width = _parse_fai(fai, self.path, self.size)
                self.fai_built = False
            else:
                self._build_fai()
                self.fai_built = True
                if write_fai:
                    self.write_fai(fai)
        except BaseException:                   # (whatever refuses the file: the mapping and the descriptor do not outlive the refusal)
            self.close()
            raise
        self.index = {n: i for i, n in enumerate(self.names)}

    # ---- the block table
    def _header(self, o):
        """(the size of the BGZF block at byte o, its ISIZE); refused when there is no whole BGZF block"""
        mm = self._mm
        if o + 28 > self.csize or mm[o:o + 4] != b"\x1f\x8b\x08\x04" or mm[o + 10:o + 16] != b"\x06\x00BC\x02\x00":
            raise BgzfReferenceError("%s: no BGZF block header at byte %d" % (self.path, o))
        size = struct.unpack_from("<H", mm, o + 16)[0] + 1
        if size < 26 or o + size > self.csize:
            raise BgzfReferenceError("%s: the BGZF block at byte %d is cut short" % (self.path, o))
        return size, struct.unpack_from("<I", mm, o + size - 4)[0]

    def _set_table(self, coff, uoff, gzi):
        """the block starts a .gzi gave (or just the first block's), completed to the end of the file by hopping over block headers
        (BSIZE, the trailer's ISIZE): nothing is inflated"""
        if gzi is not None:
            if (np.diff(coff) <= 0).any() or (np.diff(uoff) < 0).any():
                raise BgzfReferenceError("%s does not describe %s (offsets that do not increase)" % (gzi, self.path))
            if int(coff[-1]) >= self.csize:
                raise BgzfReferenceError("%s does not describe %s (an offset beyond the file)" % (gzi, self.path))
        co, uo = [], []
        o, u = int(coff[-1]), int(uoff[-1])
        while True:
            size, isize = self._header(o)
            o, u = o + size, u + isize
            if o >= self.csize:
                break
            co.append(o); uo.append(u)
        # row k: block k's start; the last row: the end of the file
        self.coff = np.concatenate([coff, np.array(co, np.int64), [o]]).astype(np.int64)
        self.uoff = np.concatenate([uoff, np.array(uo, np.int64), [u]]).astype(np.int64)
        self.n_blocks = len(self.coff) - 1
        self.size = int(self.uoff[-1])                     # of the text

    def write_gzi(self, gzi=None):
        with open(gzi or self.path + ".gzi", "wb") as f:
            f.write(gzi_bytes(self.coff[:-1], self.uoff[:-1]))

    def write_fai(self, fai=None):
        with open(fai or self.path + ".fai", "w") as f:
            f.write(self.fai_text())

    def fai_text(self):
        return "".join("%s\t%d\t%d\t%d\t%d\n" % (nm, self.length[i], self.offset[i], self.line_bases[i], self.line_width[i]) for i, nm in enumerate(self.names))

    # ---- blocks
    def _payloads(self, ks):
        """the touched blocks ks (sorted indices) as the file has them -> (comp uint8[], in_off, in_len, isize, crc), every header and
        every ISIZE checked against the table"""
        in_len = np.zeros(len(ks), np.int32)
        isize = np.zeros(len(ks), np.int32)
        crc = np.zeros(len(ks), np.uint32)
        parts = []
        for j, k in enumerate(ks.tolist()):
            o, want = int(self.coff[k]), int(self.coff[k + 1] - self.coff[k])
            size, isz = self._header(o)
            if size != want:
                raise BgzfReferenceError("%s: the BGZF block at byte %d has %d bytes, the block table says %d" % (self.path, o, size, want))
            if isz != int(self.uoff[k + 1] - self.uoff[k]):
                raise BgzfReferenceError("%s: the BGZF block at byte %d says ISIZE %d, the block table says %d" % (self.path, o, isz, int(self.uoff[k + 1] - self.uoff[k])))
            parts.append(self._mm[o + 18:o + size - 8])
            in_len[j], isize[j], crc[j] = size - 26, isz, struct.unpack_from("<I", self._mm, o + size - 8)[0]
        in_off = np.zeros(len(ks), np.int64)
        if len(ks):
            in_off[1:] = np.cumsum(in_len[:-1], dtype=np.int64)
        self.stats["blocks"] += len(ks)
        return np.frombuffer(b"".join(parts), np.uint8), in_off, in_len, isize, crc

    def _inflate_one(self, k, payload, isize, crc):
        if isize == 0:
            return b""
        try:
            d = zlib.decompress(payload, -15)
        except zlib.error as e:
            raise BgzfReferenceError("%s: the BGZF block at byte %d does not inflate (%s)" % (self.path, int(self.coff[k]), e)) from None
        if len(d) != isize or (zlib.crc32(d) & 0xFFFFFFFF) != crc:
            raise BgzfReferenceError("%s: the BGZF block at byte %d fails its CRC32 or ISIZE" % (self.path, int(self.coff[k])))
        return d

    def _inflate_host(self, ks, comp, in_off, in_len, isize, crc):
        """zlib on the host threads -> the blocks' bytes back to back (uint8[]); the verdict on a damaged block is this one's"""
        jobs = [(int(k), comp[int(o):int(o) + int(n)].tobytes(), int(z), int(c)) for k, o, n, z, c in zip(ks, in_off, in_len, isize, crc)]
        if self.threads > 1 and len(jobs) > 8:             # (a pool costs more than a few blocks; one pool serves every window)
            if self._pool is None:
                self._pool = ThreadPoolExecutor(self.threads)
            parts = list(self._pool.map(lambda j: self._inflate_one(*j), jobs))
        else:
            parts = [self._inflate_one(*j) for j in jobs]
        return np.frombuffer(b"".join(parts), np.uint8)

    def _text(self, lo, hi):
        """bytes [lo, hi) of the text (host route)"""
        if hi <= lo:
            return b""
        k0 = int(np.searchsorted(self.uoff, lo, "right")) - 1
        k1 = int(np.searchsorted(self.uoff, hi - 1, "right")) - 1
        ks = np.arange(k0, k1 + 1)
        ks = ks[np.diff(self.uoff)[ks] > 0]
        data = self._inflate_host(ks, *self._payloads(ks))
        base = int(self.uoff[ks[0]])
        return data[lo - base:hi - base].tobytes()

    # ---- the .fai when none is there
    def _build_fai(self):
        """csv_fasta_index_stream over the text, a window of blocks at a time: memory is one window, not the genome.  On the host route
        (and without a context) a window is inflated by zlib and fed as bytes.  On the device route csv_fai_events inflates it on the
        device and k_fai_events reduces it to event rows there; only the rows and the header texts come down.  A window whose rows
        or header texts exceed their buffers (stats: fai_windows_overflow), or in which the device reports a block, is fed as bytes."""
        L = lib()
        device = (self.route or DEFAULT_REF_ROUTE) == "device" and self.ctx is not None
        ptr = lambda a: a.ctypes.data if len(a) else None                          # noqa: E731
        h = L.csv_fasta_index_stream_open()
        try:
            for k0 in range(0, self.n_blocks, self.window_blocks):
                ks = np.arange(k0, min(k0 + self.window_blocks, self.n_blocks))
                comp, in_off, in_len, isize, crc = self._payloads(ks)
                if device:
                    carry, tail = np.zeros(3, np.int64), np.zeros(3, np.int64)
                    rows, hdr = np.zeros((self.fai_row_cap, 3), np.int64), np.zeros(self.fai_hdr_cap, np.uint8)
                    n_rows, hdr_bytes, status, ms = C.c_int64(0), C.c_int64(0), np.zeros(len(ks), np.uint8), (C.c_double * 2)()
                    L.csv_fasta_index_stream_carry(h, carry.ctypes.data)
                    self.ctx._check(L.csv_fai_events(self.ctx._h, ptr(comp), len(comp), len(ks), ptr(in_off), ptr(in_len), ptr(isize), ptr(crc), int(self.uoff[k0]), carry.ctypes.data,
                                                     ptr(rows), self.fai_row_cap, C.byref(n_rows), tail.ctypes.data, ptr(hdr), self.fai_hdr_cap, C.byref(hdr_bytes), ptr(status), ms))
                    self.stats["ms_fai_inflate"] += ms[0]
                    self.stats["ms_fai_events"] += ms[1]
                    if n_rows.value < 0:
                        self.stats["fai_windows_host_after_device"] += 1       # the host inflates the window again: its verdict stands
                    elif n_rows.value > self.fai_row_cap or hdr_bytes.value > self.fai_hdr_cap:
                        self.stats["fai_windows_overflow"] += 1
                    else:
                        self.stats["fai_windows_device"] += 1
                        self.stats["fai_rows"] += n_rows.value
                        if L.csv_fasta_index_stream_rows(h, ptr(rows), n_rows.value, ptr(hdr), hdr_bytes.value, int(isize.sum()), tail.ctypes.data) != _abi.OK:
                            break
                        continue
                data = self._inflate_host(ks, comp, in_off, in_len, isize, crc)
                self.stats["fai_windows_host"] += 1
                if L.csv_fasta_index_stream_feed(h, data.ctypes.data if len(data) else None, len(data)) != _abi.OK:
                    break
            cap, ncap = 1024, 1 << 16
            while True:
                names = np.zeros(ncap, np.uint8)
                nb = C.c_int64(0)
                name_off, name_len = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
                length, offset = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
                lb, lw = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
                n = L.csv_fasta_index_stream_finish(h, cap, names.ctypes.data, ncap, C.byref(nb), name_off.ctypes.data, name_len.ctypes.data, length.ctypes.data,
                                                    offset.ctypes.data, lb.ctypes.data, lw.ctypes.data)
                if n < 0:
                    raise ValueError("%s cannot be indexed (sequence before a header, or lines of unequal length inside a contig)" % self.path)
                if n <= cap and nb.value <= ncap:
                    break
                cap, ncap = max(cap, int(n)), max(ncap, int(nb.value))
        finally:
            L.csv_fasta_index_stream_close(h)
        self.names = [names[int(name_off[i]):int(name_off[i]) + int(name_len[i])].tobytes().decode() for i in range(n)]
        self.length, self.offset, self.line_bases, self.line_width = length[:n], offset[:n], lb[:n], lw[:n]

    # ---- access
    def __contains__(self, name):
        return name in self.index

    def fetch(self, name, start=0, end=None):
        """bases [start, end) of a contig as str (pysam.FastaFile.fetch), on the host route; for tests and small slices"""
        i = self.index[name]
        n, lb, lw, off = int(self.length[i]), int(self.line_bases[i]), int(self.line_width[i]), int(self.offset[i])
        end = n if end is None else min(end, n)
        start = max(0, start)
        if end <= start:
            return ""
        lo = off + (start // lb) * lw + start % lb
        hi = off + ((end - 1) // lb) * lw + (end - 1) % lb + 1
        return self._text(lo, hi).replace(b"\r", b"").replace(b"\n", b"").decode()

    def gather(self, name_idx, beg, end, ctx=None, route=None, timings=None):
        """bases [beg[r], end[r]) of contig name_idx[r] (an index into names), for all r -> (blob uint8[], off int64[n + 1]): the raw
        bytes of the ranges back to back, line breaks removed.  Only the blocks the ranges touch are read from the file, in windows
        of at most window_blocks of them, cut between ranges taken in the order of their first block.  route: "host", "device" (ctx: an engine.Context; default: the one
        given at construction) or None (the route given at construction, else DEFAULT_REF_ROUTE).  On the device route a window in
        which the device reports a block with a non-zero status is served by the host route, whose verdict stands.
        timings (a dict): ms_inflate / ms_gather grow by the kernels' time."""
        route = route or self.route or DEFAULT_REF_ROUTE
        if route not in REF_ROUTES:
            raise ValueError("route must be one of %s, not %r" % (", ".join(REF_ROUTES), route))
        ctx = ctx if ctx is not None else self.ctx
        if route == "device" and ctx is None:
            raise ValueError("the device route needs a context: gather(..., ctx=<engine.Context>)")
        ci = np.ascontiguousarray(name_idx, np.int64).reshape(-1)
        beg, end = np.ascontiguousarray(beg, np.int64).reshape(-1), np.ascontiguousarray(end, np.int64).reshape(-1)
        n = len(ci)
        if not (len(beg) == len(end) == n):
            raise ValueError("gather: name_idx, beg and end must have one length")
        off = np.zeros(n + 1, np.int64)
        if n == 0:
            return np.zeros(0, np.uint8), off
        if (ci < 0).any() or (ci >= len(self.names)).any():
            raise ValueError("gather: a contig index outside the %d contigs of %s" % (len(self.names), self.path))
        clen = np.asarray(self.length, np.int64)[ci]
        bad = np.flatnonzero((beg < 0) | (end < beg) | (end > clen))
        if len(bad):
            r = int(bad[0])
            raise ValueError("gather: range %d, [%d, %d), does not lie inside contig %s of %d bases" % (r, beg[r], end[r], self.names[int(ci[r])], clen[r]))
        base_off = np.ascontiguousarray(np.asarray(self.offset, np.int64)[ci])
        lb = np.ascontiguousarray(np.asarray(self.line_bases, np.int32)[ci])
        lw = np.ascontiguousarray(np.asarray(self.line_width, np.int32)[ci])
        np.cumsum(end - beg, out=off[1:])
        has = end > beg
        # (an empty range reads nothing: a contig without sequence has no line length to give it)
        lb, lw = np.where(has, lb, 1).astype(np.int32), np.where(has, lw, 1).astype(np.int32)
        lbs = np.maximum(lb, 1).astype(np.int64)
        lo = base_off + (beg // lbs) * lw + beg % lbs
        hi = base_off + ((end - 1) // lbs) * lw + (end - 1) % lbs          # the last source byte
        kf = np.where(has, np.searchsorted(self.uoff, lo, "right") - 1, 0)
        kl = np.where(has, np.searchsorted(self.uoff, hi, "right") - 1, -1)
        blob = np.empty(int(off[-1]), np.uint8)
        nonempty = np.diff(self.uoff) > 0
        # The ranges are served in the order of their first block, so that a window's ranges share their blocks and a block is
        # inflated in about one window, whatever order the caller asks in; the result is in the caller's order.
        order = np.argsort(kf, kind="stable")
        in_order = bool((order[1:] > order[:-1]).all())
        first, kl_o = kf[order], kl[order]
        last = np.maximum.accumulate(kl_o)                             # of every range up to this one
        length = end - beg
        j0 = 0
        while j0 < n:
            # ranges order[j0 : j1]: as many as lie within window_blocks blocks from the first one's first block (one range at least).
            # A range of an earlier window that reached further than this window may (a DEL across more than window_blocks blocks)
            # must not shorten the windows behind it: the running maximum restarts at the window's first range then.
            if j0 and int(last[j0 - 1]) > int(first[j0]) + self.window_blocks - 1:
                last[j0:] = np.maximum.accumulate(kl_o[j0:])
            j1 = max(int(np.searchsorted(last[j0:], int(first[j0]) + self.window_blocks - 1, "right")) + j0, j0 + 1)
            w = slice(j0, j1) if in_order else order[j0:j1]
            ln = length[w]
            if int(ln.sum()) > 0:
                mark = np.zeros(self.n_blocks + 1, np.int32)
                np.add.at(mark, kf[w][has[w]], 1)
                np.add.at(mark, kl[w][has[w]] + 1, -1)
                ks = np.flatnonzero((np.cumsum(mark[:-1]) > 0) & nonempty)
                out = self._window(ks, np.ascontiguousarray(base_off[w]), np.ascontiguousarray(lb[w]), np.ascontiguousarray(lw[w]), np.ascontiguousarray(beg[w]),
                                   np.ascontiguousarray(end[w]), route, ctx, timings)
                if in_order:
                    blob[int(off[j0]):int(off[j1])] = out
                else:                                          # single bases in one indexed store, the longer ranges slice by slice
                    src = np.zeros(len(ln) + 1, np.int64)
                    np.cumsum(ln, out=src[1:])
                    dst = off[:-1][w]
                    one = ln == 1
                    blob[dst[one]] = out[src[:-1][one]]
                    for j in np.flatnonzero(ln > 1).tolist():
                        blob[int(dst[j]):int(dst[j]) + int(ln[j])] = out[int(src[j]):int(src[j + 1])]
            j0 = j1
        return blob, off

    def _window(self, ks, base_off, lb, lw, beg, end, route, ctx, timings):
        L = lib()
        comp, in_off, in_len, isize, crc = self._payloads(ks)
        uoff = np.ascontiguousarray(self.uoff[ks])
        n = len(beg)
        total = int((end - beg).sum())
        out, out_off, need = np.empty(total, np.uint8), np.zeros(n + 1, np.int64), C.c_int64(-1)
        ptr = lambda a: a.ctypes.data if len(a) else None                          # noqa: E731
        if route == "device":
            status, ms = np.zeros(len(ks), np.uint8), (C.c_double * 2)()
            rc = L.csv_ref_gather(ctx._h, ptr(comp), len(comp), len(ks), ptr(in_off), ptr(in_len), ptr(uoff), ptr(isize), ptr(crc), n, ptr(base_off), ptr(lb), ptr(lw), ptr(beg),
                                  ptr(end), ptr(out), total, out_off.ctypes.data, C.byref(need), ptr(status), 0, ms)
            ctx._check(rc)
            if timings is not None:
                timings["ms_inflate"] = timings.get("ms_inflate", 0.0) + ms[0]
                timings["ms_gather"] = timings.get("ms_gather", 0.0) + ms[1]
            if not status.any():
                if need.value != total:
                    raise RuntimeError("csv_ref_gather: %d bytes where %d were asked for" % (need.value, total))
                self.stats["windows_device"] += 1
                return out
            self.stats["windows_host_after_device"] += 1       # the host inflates the window again: its verdict stands
        data = self._inflate_host(ks, comp, in_off, in_len, isize, crc)
        data_off = np.zeros(len(ks), np.int64)
        if len(ks):
            data_off[1:] = np.cumsum(isize[:-1], dtype=np.int64)
        err = C.create_string_buffer(512)
        rc = L.csv_ref_gather_host(ptr(data), len(data), len(ks), ptr(data_off), ptr(uoff), ptr(isize), n, ptr(base_off), ptr(lb), ptr(lw), ptr(beg), ptr(end), ptr(out), total,
                                   out_off.ctypes.data, C.byref(need), err, len(err))
        if rc != _abi.OK or need.value != total:
            raise BgzfReferenceError("%s: %s" % (self.path, err.value.decode() or "csv_ref_gather_host failed (%s)" % _abi.ERR_NAME.get(rc, rc)))
        self.stats["windows_host"] += 1
        return out

    def close(self):
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None
        if self._mm is not None:
            self._mm.close()
            self._mm = None
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_fasta(path, only=None):
    """{contig name: sequence} with every contig as one str (plain or gzip): the round-1 reader, for gzip files and tests"""
    opener = gzip.open if str(path).endswith(".gz") else open
    out, name, parts = {}, None, []
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                if name is not None and (only is None or name in only):
                    out[name] = "".join(parts)
                name, parts = line[1:].split()[0], []
            elif name is not None and (only is None or name in only):
                parts.append(line.strip())
    if name is not None and (only is None or name in only):
        out[name] = "".join(parts)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cutesv_amd.fasta", description="index a FASTA file, plain or BGZF-compressed, like `samtools faidx`")
    ap.add_argument("file")
    ap.add_argument("--faidx", action="store_true", required=True, help="build the .fai (and, of a BGZF file, the .gzi)")
    ap.add_argument("--write", action="store_true", help="write FILE.fai (and FILE.gzi) beside the file; without it the .fai is printed")
    ap.add_argument("--route", choices=REF_ROUTES, default="host", help="where the text of a BGZF file is inflated and its lines are found (device: on GPU 0)")
    ap.add_argument("-t", "--threads", type=int, default=HOST_THREADS, help="zlib threads of the host route")
    a = ap.parse_args(argv)
    kind = sniff(a.file)
    if kind == "gzip":
        ap.error("%s is gzip-compressed but has no BGZF blocks: compress it with bgzip" % a.file)
    # (an index beside the file is not trusted here: this command makes them)
    none = os.path.join(os.path.dirname(os.path.abspath(a.file)), ".no-such-index")
    if kind == "bgzf":
        ctx = None
        if a.route == "device":
            from . import engine
            ctx = engine.Context(0)
        try:
            ref = BgzfReference(a.file, fai=none, gzi=none, ctx=ctx, route=a.route, threads=a.threads)
        finally:
            if ctx is not None:
                ctx.close()
        text = ref.fai_text()
        if a.write:
            ref.write_fai()
            ref.write_gzi()
        st = ref.stats
        print("cutesv_amd.fasta: %d contigs, %d bases, %d BGZF blocks, windows: %d on the device (%d rows), %d on the host (%d of them beyond the row buffer)%s"
              % (len(ref.names), int(np.sum(ref.length)), ref.n_blocks, st["fai_windows_device"], st["fai_rows"], st["fai_windows_host"], st["fai_windows_overflow"],
                 ": %s.fai and %s.gzi written" % (a.file, a.file) if a.write else ""), file=sys.stderr)
    else:
        ref = Reference(a.file, fai=none)
        text = "".join("%s\t%d\t%d\t%d\t%d\n" % (nm, ref.length[i], ref.offset[i], ref.line_bases[i], ref.line_width[i]) for i, nm in enumerate(ref.names))
        if a.write:
            ref.write_fai(a.file + ".fai")
        print("cutesv_amd.fasta: %d contigs, %d bases%s" % (len(ref.names), int(np.sum(ref.length)), ": %s.fai written" % a.file if a.write else ""), file=sys.stderr)
    ref.close()
    if not a.write:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
