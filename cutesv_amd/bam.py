"""Native BAM reader: a coordinate-sorted .bam -> the columns the extraction kernels take, without
pysam and without a Python object per record.

`BamFile` is the host side (cutesv_amd/csrc/bam_host.cpp: BGZF inflate on host threads with the interpreter lock released - or,
with inflate=<Context>, on the device, one wavefront per block - header, record framing, region scan;
with a .bai beside the file a region's scan starts at its linear-index entry, without one at the contig).  It hands out `Chunk`s: the slim image that goes to the device (per
record the 32 fixed bytes, the CIGAR words and the aux bytes) and the host image that stays behind (read names and 4-bit
sequences, sliced only for the records somebody asks for).  `decode(ctx, chunk)` is the face of `csv_bam_decode`
(bam.hip.h); `decode_host(chunk)` is the same function in numpy / Python - the CPU path, and what the tests compare the
kernels with.

`inflate_blocks(ctx, payloads, isizes, crcs)` is the face of `csv_bgzf_inflate`, `inflate_blocks_host` its twin on Python's zlib.

With frame="device"  the inflated window stays on the device as well: the records are framed there, a
`FramedChunk` keeps its two images in the context's device memory (`slim` / `host` fetch them on first access), and `decode`,
`rebuild.name_pool_append_chunk` and `extract.upload_read_sequences` take them where they lie.

A file without a .bai gets one from `BamFile.build_index`: one pass over the file on the reader's routes -
with frame="device" the index kernels work on the rows of every window, which stay on the device - and the bytes of a .bai
file (SAMv1 5.2, htslib's conventions).  `BamFile(path, index="build")` loads the index beside the file when there is one and builds one in memory otherwise.
A .csi beside the file (`index_format`) serves as a .bai does, and `build_index(format="csi")` builds one: the
index a file with a contig of 2^29 bases or more needs.

    python -m cutesv_amd.bam FILE [--chrom C] [--dump-columns DIR] [--inflate {host,device}] [--frame {host,device}] [--idxstats]
    python -m cutesv_amd.bam FILE --index [--csi [--min_shift N]] [--index_out PATH] [--force] [--inflate {host,device}] [--frame {host,device}]
    python -m cutesv_amd.bam FILE --sort -o OUT [--index [--csi]] [--force] [--sort_route {host,device}] [--max_bytes N] [--inflate {host,device}] [--frame {host,device}]

`sort_bam` sorts a file by coordinate - what an aligner writes goes straight in: the inflated stream stays in device
memory, the keys are sorted by the rebuild's radix passes, k_sort_gather moves every byte once into sorted order and the device
compressor writes the BGZF blocks; `sort_bam_host_twin` is the same on the host.  It is the one place that opens a file whose header
does not say SO:coordinate.
"""
import ctypes as C
import os
import tempfile
import time
import zlib

import numpy as np

from . import _abi
from ._abi import ChunkC, BamIn, BamOut, BAM_OUT as _OUT, BAM_DEV as _DEV      # noqa: F401  (the mirrors live in _abi)
from ._lib import lib

ALL = 1 << 62                              # "no bound" of a region


class BamError(ValueError):
    pass


def default_threads():
    """host threads of the inflate: min(16, CPUs), the rule phase3 uses - never the whole machine's count"""
    return max(1, min(16, os.cpu_count() or 1))


def _from_ptr(ptr, count, dtype):
    """a copy of `count` items of `dtype` at address `ptr` (the reader's arrays live only until its next call)"""
    if not count:
        return np.zeros(0, dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype, count).copy()


_NIBBLE = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)


class Chunk:
    """the records one csv_bam_read handed out: `slim` / `rec_off` / `rec_len` go to the device, `host` / `host_off` stay"""

    def __init__(self, chrom, refid, slim, rec_off, rec_len, host, host_off, more, stats):
        self.chrom, self.refid, self.more, self.stats = chrom, refid, more, stats
        self.slim, self.rec_off, self.rec_len, self.host, self.host_off = slim, rec_off, rec_len, host, host_off
        self.n = len(rec_off)

    def __len__(self):
        return self.n

    def _name_len(self, i):
        return int(self.slim[int(self.rec_off[i]) + 8])                       # l_read_name, NUL included

    def name_columns(self):
        """-> (off int64[n], len int32[n]): name i is host[off[i] : off[i] + len[i]] - the strided form csv_name_pool_append
        takes, with `host` as its bytes: no name is sliced or copied here"""
        n_len = self.slim[self.rec_off + 8].astype(np.int32) if self.n else np.zeros(0, np.int32)      # l_read_name, NUL included
        return np.ascontiguousarray(self.host_off[:self.n], np.int64), np.maximum(n_len - 1, 0)

    def sequence_columns(self):
        """-> (off int64[n], l_seq int32[n]): the bases of record i are the (l_seq[i] + 1) // 2 bytes at host[off[i]:], 4 bits per
        base, high nibble first - the strided form csv_seq_reads_upload takes, with `host` as its bytes: nothing is decoded here"""
        if not self.n:
            return np.zeros(0, np.int64), np.zeros(0, np.int32)
        fixed = self.rec_off[:, None] + np.arange(16, 20)                      # l_seq: bytes 16 .. 19 of a record, little endian
        l_seq = np.ascontiguousarray(self.slim[fixed]).view("<u4").ravel().astype(np.int32)
        n_len = self.slim[self.rec_off + 8].astype(np.int64)                   # l_read_name, NUL included
        return np.ascontiguousarray(self.host_off[:self.n], np.int64) + n_len, l_seq

    def name(self, i):
        h0 = int(self.host_off[i])
        return self.host[h0 : h0 + self._name_len(i) - 1].tobytes().decode()

    def sequence(self, i):
        """the query sequence of record i, decoded from its 4 bits per base"""
        off = int(self.rec_off[i])
        l_seq = int(self.slim[off + 16 : off + 20].view(np.uint32)[0])
        h0 = int(self.host_off[i]) + self._name_len(i)
        packed = self.host[h0 : h0 + (l_seq + 1) // 2]
        both = np.empty(2 * len(packed), np.uint8)
        both[0::2] = packed >> 4
        both[1::2] = packed & 15
        return _NIBBLE[both[:l_seq]].tobytes().decode()

    def text(self, beg, end):
        """bytes [beg, end) of the slim image as text (an SA value)"""
        return self.slim[int(beg) : int(end)].tobytes().decode()

    def sa_values(self, cols, i):
        """the values of record i's SA tags, in tag order"""
        return [self.text(cols["sa_beg"][k], cols["sa_end"][k]) for k in range(int(cols["sa_off"][i]), int(cols["sa_off"][i + 1]))]


class FramedChunk(Chunk):
    """a Chunk of the framing route (frame="device"): the two images lie in the context's device memory, where `decode`,
    `rebuild.name_pool_append_chunk` and `extract.upload_read_sequences` take them.  `slim` and `host` fetch both on first access
    (csv_bam_chunk_fetch) - for checks and for the rare host fallbacks.  The device images live until the reader's next read or
    route change: a fetch or a framed consumer after that raises."""

    framed = True

    def __init__(self, bamfile, chrom, refid, rec_off, rec_len, host_off, l_name, l_seq, more, stats, slim_bytes, host_bytes):
        self._bf, self._serial, self._images = bamfile, bamfile._read_serial, None
        self._l_name, self._l_seq, self._bytes = l_name, l_seq, (slim_bytes, host_bytes)
        Chunk.__init__(self, chrom, refid, None, rec_off, rec_len, None, host_off, more, stats)

    @property
    def ctx(self):
        return self._bf.frame

    @property
    def slim_bytes(self):
        return self._bytes[0]

    def valid(self):
        """the device images are still this chunk's"""
        return self._bf._h and self._bf.frame is not None and self._bf._read_serial == self._serial

    def check(self):
        if not self.valid():
            raise BamError("%s: the device chunk is gone: it lives until the reader's next read or route change" % self._bf.path)

    def _fetch(self):
        if self._images is None:
            self.check()
            slim, host = np.empty(self._bytes[0], np.uint8), np.empty(self._bytes[1], np.uint8)
            rc = self._bf._L.csv_bam_chunk_fetch(self._bf._h, slim.ctypes.data if len(slim) else None, host.ctypes.data if len(host) else None)
            if rc:
                raise BamError("%s: %s" % (self._bf.path, self._bf._error_text()))
            self._images = (slim, host)
        return self._images

    slim = property(lambda self: self._fetch()[0], lambda self, v: None)
    host = property(lambda self: self._fetch()[1], lambda self, v: None)

    @property
    def fetched(self):
        return self._images is not None

    def _name_len(self, i):
        return int(self._l_name[i])

    def name_columns(self):
        return np.ascontiguousarray(self.host_off[:self.n], np.int64), np.maximum(self._l_name - 1, 0).astype(np.int32)

    def sequence_columns(self):
        return np.ascontiguousarray(self.host_off[:self.n], np.int64) + self._l_name.astype(np.int64), self._l_seq.copy()


class BamFile:
    """A coordinate-sorted BAM file.  `.references`, `.lengths`, `.header_text`; `.chunks(chrom)` iterates a contig in file
    order, `.records(chrom, start, end)` returns the records that overlap a region (what pysam's fetch yields), found by
    a forward scan that stops at the first record starting at or after `end`: no index file is needed.  With an index
    (`has_index`) the scan starts at the linear-index entry of `start`; what it yields is the same, byte for byte."""

    def __init__(self, path, threads=None, inflate=None, index=None, frame=None, _any_order=False):
        """frame: None or "host" - the records are framed on the host; "device" - on the device of `inflate`, which must be a
        Context (set_frame).
        inflate: None or "host" - the BGZF blocks are inflated on `threads` host threads; an engine.Context - on its device
        (set_inflate).  The header is read on the host either way.
        index: None - <path>.bai, else <path minus .bam>.bai, is loaded when there is one; a path - that index, which must exist;
        False - none; "build" - the index beside the file when there is one, else one is built in memory on the routes given
        (build_index; nothing is written).  An index that is found and does not validate against this file raises BamError."""
        _frame_route(frame, _inflate_ctx(inflate))                           # (refused before the file is opened)
        L = self._L = lib()
        self._h = C.c_void_p()
        self.inflate, self.last_stats, self.window_blocks = None, {}, 0
        self.frame, self._read_serial = None, 0
        self.threads = default_threads() if threads is None else max(1, int(threads))
        err = C.create_string_buffer(512)
        rc = L.csv_bam_open(os.fsencode(path), self.threads, C.byref(self._h), err, len(err))
        if rc:
            self._h = C.c_void_p()
            raise BamError("%s: %s" % (path, err.value.decode(errors="replace") or "cannot be read"))
        n_ref, names, lengths, text, text_len = C.c_int32(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        L.csv_bam_header(self._h, C.byref(n_ref), C.byref(names), C.byref(lengths), C.byref(text), C.byref(text_len))
        self.header_text = C.string_at(text.value, text_len.value).decode(errors="replace") if text_len.value else ""
        self.lengths = _from_ptr(lengths.value, n_ref.value, np.int64).tolist()
        self.references, p = [], names.value
        for _ in range(n_ref.value):
            s = C.string_at(p)
            self.references.append(s.decode()); p += len(s) + 1
        self._refid = {r: i for i, r in enumerate(self.references)}
        self.path = path
        hd = [ln for ln in self.header_text.split("\n") if ln.startswith("@HD")]
        so = [f[3:] for ln in hd for f in ln.split("\t") if f.startswith("SO:")]
        self.sort_order = so[0] if so else None
        if self.sort_order != "coordinate" and not _any_order:              # (_any_order: sort_bam's own reader, and nobody else's)
            self.close()
            raise BamError("%s: the header says SO:%s; a coordinate-sorted file is needed (samtools sort)" % (path, self.sort_order or "<missing>"))
        self.set_inflate(inflate)
        self.set_frame(frame)
        self.has_index = False
        self.index_stats = None
        self.index_format = None
        build = isinstance(index, str) and index == "build"
        if index is not False:
            try:
                self.load_index(None if index is None or index is True or build else index, required=index is not None and not build)
                if build and not self.has_index:
                    self.build_index()
            except BamError:
                self.close()
                raise

    def _error_text(self):
        """csv_bam_error: what the reader said about its last failure"""
        return (self._L.csv_bam_error(self._h) or b"").decode(errors="replace")

    def load_index(self, path=None, required=True):
        """csv_bam_index_load: path None tries <bam>.bai, <bam minus .bam>.bai, then the same two names with .csi.  The format is
        told by the file's content (index_format: "bai" or "csi").  -> has_index.  BamError: the index does
        not validate (a reader whose load failed has none), or - with required - there is no such file."""
        rc = self._L.csv_bam_index_load(self._h, None if path is None else os.fsencode(path))
        if rc == _abi.E_STATE and not required:
            return self.has_index
        if rc:
            self.has_index, self.index_format = False, None
            raise BamError(self._error_text() or "%s: the index cannot be loaded" % self.path)
        self.has_index = True
        self._index_format()
        return True

    def _index_format(self):
        self.index_format = {1: "bai", 2: "csi"}.get(int(self._L.csv_bam_index_format(self._h))) if self.has_index else None

    def build_index(self, write=None, overwrite=False, format="bai", min_shift=14, depth=None):
        """format "csi": csv_bam_index_build_csi - a CSI index of 2^min_shift-base windows and `depth` levels (None: htslib's rule,
        the smallest that holds the longest reference), the only kind a file with a contig of 2^29 bases or more can have; write=True
        then goes to <path>.csi and index_bytes() gives the .csi file, index_payload() what it inflates to; the stats gain `bins` and
        `ms_loff`, the device time of k_index_loff.
        csv_bam_index_build: one pass over the whole file on the reader's current routes -> the index is installed (has_index)
        and the stats dict is returned: records, runs, index_bytes, ms (wall), ms_kernels, bytes_up, bytes_down, frame_runs,
        index_windows, inflate / frame (the routes) and their block counters.  write: True - the bytes also go to <path>.bai; a path
        - there; through a temporary file beside the target and os.replace.  FileExistsError, before anything is read, when the
        target exists and overwrite is not set.  BamError: a record the BAI format cannot index or that is out of order (the text
        names the file and the record's ordinal), or what the reader refuses; nothing is installed and nothing is written.  The
        build counts as a read: a FramedChunk handed out before it is dead."""
        if format not in ("bai", "csi"):
            raise ValueError("format is \"bai\" or \"csi\", not %r" % (format,))
        target = None
        if write is not None and write is not False:
            target = os.fspath(self.path) + "." + format if write is True else os.fspath(write)
            if os.path.exists(target) and not overwrite:
                raise FileExistsError("%s exists (overwrite=True replaces it)" % target)
        self._read_serial += 1
        n, t0 = C.c_int64(), time.perf_counter()
        if format == "csi":
            rc = self._L.csv_bam_index_build_csi(self._h, int(min_shift), 0 if depth is None else int(depth), C.byref(n))
        else:
            rc = self._L.csv_bam_index_build(self._h, 0, C.byref(n))
        ms = (time.perf_counter() - t0) * 1e3
        if rc:
            text = self._error_text()
            if format == "bai" and "which the BAI format cannot index" in text:
                text += ".  A CSI index has no such limit: build_index(format=\"csi\"), --index --csi on the command line"
            raise BamError("%s: %s" % (self.path, text))
        self.has_index = True
        self._index_format()
        v = [C.c_int64() for _ in range(6)]
        msk = C.c_double()
        self._L.csv_bam_index_build_stats(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(msk), C.byref(v[2]), C.byref(v[3]), C.byref(v[4]), C.byref(v[5]))
        stats = dict(format=format, records=int(v[0].value), runs=int(v[1].value), index_bytes=int(n.value), ms=ms, ms_kernels=float(msk.value), bytes_up=int(v[2].value),
                     bytes_down=int(v[3].value), frame_runs=int(v[4].value), index_windows=int(v[5].value), written=None)
        if format == "csi":
            bins, ms_loff = C.c_int64(), C.c_double()
            self._L.csv_bam_index_build_stats_csi(self._h, C.byref(bins), C.byref(ms_loff))
            stats.update(bins=int(bins.value), ms_loff=float(ms_loff.value))
        stats.update(self.inflate_stats())
        stats.update(self.frame_stats())
        if target is not None:
            data = self.index_bytes()
            fd, tmp = tempfile.mkstemp(prefix=os.path.basename(target) + ".", suffix=".tmp", dir=os.path.dirname(target) or ".")
            try:
                with os.fdopen(fd, "wb") as f:
                    f.write(data)
                os.replace(tmp, target)
            except BaseException:
                if os.path.exists(tmp):
                    os.unlink(tmp)
                raise
            stats["written"] = target
        self.index_stats = stats
        return stats

    def index_payload(self):
        """what the .csi file of a BUILT CSI index inflates to (csv_bam_index_payload).  BamError: the reader holds no built CSI index"""
        need = C.c_int64()
        rc = self._L.csv_bam_index_payload(self._h, None, 0, C.byref(need))
        if rc != _abi.E_CAPACITY:
            raise BamError("%s: the reader holds no built CSI index (build_index(format=\"csi\"))" % self.path)
        buf = np.empty(int(need.value), np.uint8)
        if self._L.csv_bam_index_payload(self._h, buf.ctypes.data, len(buf), C.byref(need)):
            raise BamError("%s: the built index cannot be fetched" % self.path)
        return buf.tobytes()

    def index_bytes(self):
        """the bytes of a BUILT index, as a .bai or .csi file holds them (csv_bam_index_bytes).  BamError: the reader has no index, or one
        loaded from a file (its bins were not kept)"""
        need = C.c_int64()
        rc = self._L.csv_bam_index_bytes(self._h, None, 0, C.byref(need))
        if rc != _abi.E_CAPACITY:
            raise BamError("%s: the reader holds no built index (build_index; a loaded index keeps no bins)" % self.path)
        buf = np.empty(int(need.value), np.uint8)
        rc = self._L.csv_bam_index_bytes(self._h, buf.ctypes.data, len(buf), C.byref(need))
        if rc:
            raise BamError("%s: the built index cannot be fetched" % self.path)
        return buf.tobytes()

    def index_block(self, chrom, pos):
        """the number of the BGZF block in which a read of `chrom` from `pos` on starts (its linear-index entry); -1: the index says
        that nothing is there.  BamError without an index."""
        k = int(self._L.csv_bam_index_block(self._h, self.refid(chrom), int(pos)))
        if k < -1:
            raise BamError("%s: no index is loaded" % self.path)
        return k

    def drop_index(self):
        self._L.csv_bam_index_drop(self._h)
        self.has_index, self.index_format = False, None

    def _index_counts(self):
        if not self.has_index:
            raise BamError("%s: no index is loaded" % self.path)
        n = len(self.references)
        mapped, unmapped, nc = np.zeros(n, np.int64), np.zeros(n, np.int64), C.c_int64()
        self._L.csv_bam_index_stats(self._h, mapped.ctypes.data if n else None, unmapped.ctypes.data if n else None, C.byref(nc))
        return mapped, unmapped, int(nc.value)

    def index_statistics(self):
        """[(contig, mapped, unmapped, total)] in header order: the counts of the index's pseudo-bins, what pysam's
        get_index_statistics gives (zeros for a contig without one)"""
        mapped, unmapped, _ = self._index_counts()
        return [(c, int(m), int(u), int(m + u)) for c, m, u in zip(self.references, mapped, unmapped)]

    @property
    def no_coordinate(self):
        """n_no_coor of the index: the reads without coordinates (None: the index does not carry it)"""
        nc = self._index_counts()[2]
        return None if nc < 0 else nc

    def set_inflate(self, inflate, window_blocks=None):
        """Where the BGZF blocks are inflated from now on: None or "host" - host threads; an engine.Context - csv_bgzf_inflate on
        its device, window_blocks blocks per call (0: the library's default; None: what this reader was last told), with the host
        inflating again whatever block the device gives up on.  What a chunk contains does not depend on it.  -> the previous
        setting (None or the Context).  The Context must stay open as long as it is set here."""
        ctx = _inflate_ctx(inflate)
        window_blocks = self.window_blocks if window_blocks is None else window_blocks
        if not isinstance(window_blocks, (int, np.integer)) or not 0 <= int(window_blocks) <= 16384:
            raise ValueError("window_blocks must lie in 0 .. 16384, not %r" % (window_blocks,))
        rc = self._L.csv_bam_set_inflate(self._h, ctx._h if ctx is not None else None, int(window_blocks))
        if rc:
            raise BamError("%s: the inflate route cannot be set" % self.path)
        prev, self.inflate, self.window_blocks = self.inflate, ctx, int(window_blocks)
        self.frame, self._read_serial = None, self._read_serial + 1              # (the library switches back to host framing with the inflate route)
        return prev

    def set_frame(self, frame):
        """Where the records are framed from now on: None or "host" - on the host, out of the inflated window; "device" - on the
        device of the inflate route (csv_bam_set_frame; ValueError when the blocks are inflated on the host): the window, the slim
        image and the host image stay in device memory and the reader hands out FramedChunks.  What a chunk contains does not
        depend on it.  -> the previous setting ("host" or "device")."""
        route = _frame_route(frame, self.inflate)
        rc = self._L.csv_bam_set_frame(self._h, self.inflate._h if route == "device" else None)
        if rc:
            self.frame, self._read_serial = None, self._read_serial + 1          # (a reader that was refused frames on the host)
            raise BamError("%s: %s" % (self.path, self._error_text()))
        prev, self.frame = "host" if self.frame is None else "device", self.inflate if route == "device" else None
        self._read_serial += 1
        return prev

    def frame_stats(self, zero=False):
        """of the last read: dict(frame "host" | "device", right_blocks, frame_fallback_blocks, ms_frame_kernels, frame_bytes_down, frame_bytes_up).
        zero: of a read that did not reach the library - the route and zero counters"""
        r, f, ms, dn, up = C.c_int64(), C.c_int64(), C.c_double(), C.c_int64(), C.c_int64()
        if not zero:
            self._L.csv_bam_frame_stats(self._h, C.byref(r), C.byref(f), C.byref(ms), C.byref(dn), C.byref(up))
        return dict(frame="host" if self.frame is None else "device", right_blocks=int(r.value), frame_fallback_blocks=int(f.value), ms_frame_kernels=float(ms.value),
                    frame_bytes_down=int(dn.value), frame_bytes_up=int(up.value))

    def inflate_stats(self, zero=False):
        """of the last read: dict(inflate "host" | "device", device_blocks, fallback_blocks, ms_inflate_kernels); zero: as in frame_stats"""
        dev, fb, ms = C.c_int64(), C.c_int64(), C.c_double()
        if not zero:
            self._L.csv_bam_inflate_stats(self._h, C.byref(dev), C.byref(fb), C.byref(ms))
        return dict(inflate="host" if self.inflate is None else "device", device_blocks=int(dev.value), fallback_blocks=int(fb.value), ms_inflate_kernels=float(ms.value))

    def close(self):
        if self._h:
            if self.frame is not None and self.frame._h:      # (the context's one framing reader leaves before it goes)
                self._L.csv_bam_set_frame(self._h, None)
            self.frame = None
            self._L.csv_bam_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def refid(self, chrom):
        """chrom: a reference name, or None for the unmapped tail (refID -1)"""
        if chrom is None:
            return -1
        if chrom not in self._refid:
            raise KeyError("no reference %r in %s" % (chrom, self.path))
        return self._refid[chrom]

    def _read(self, chrom, beg, end, max_records, flags, ranges=None):
        cc = ChunkC()
        refid = self.refid(chrom)
        self._read_serial += 1
        count_only = bool(flags & _abi.BAM_COUNT_ONLY)
        empty = ranges is not None and len(ranges) == 0        # nothing to read: the library is not asked, no block is touched, `cc` stays zero
        if empty:
            rc = 0
        elif ranges is None:
            rc = self._L.csv_bam_read(self._h, refid, int(beg), int(end), int(max_records), int(flags), C.byref(cc))
        else:
            rc = self._L.csv_bam_read_ranges(self._h, refid, len(ranges), ranges[:, 0].ctypes.data, ranges[:, 1].ctypes.data, int(max_records), int(flags), C.byref(cc))
        if rc:
            raise BamError("%s: %s" % (self.path, self._error_text()))
        n = int(cc.n_records)
        stats = dict(n_records=n, record_bytes=int(cc.record_bytes), inflated_bytes=int(cc.inflated_bytes), compressed_bytes=int(cc.compressed_bytes),
                     slim_bytes=int(cc.slim_bytes), ms_inflate=float(cc.ms_inflate), ms_frame=float(cc.ms_frame))
        stats.update(self.inflate_stats(zero=empty))
        if self.frame is not None:
            stats.update(self.frame_stats(zero=empty))
        self.last_stats = stats
        if count_only and not empty:
            return n, bool(cc.more)
        # bytes that cross PCIe per record (image + offset + length) next to the inflated bytes of the record
        stats["upload_bytes_per_record"] = (int(cc.slim_bytes) + 12 * n) / n if n else 0.0
        stats["inflated_bytes_per_record"] = int(cc.record_bytes) / n if n else 0.0
        if empty:                                              # the empty chunk (a plain one on every route: it has no image anywhere)
            return (0, False) if count_only else Chunk(chrom, refid, np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint8),
                                                       np.zeros(1, np.int64), False, stats)
        if self.frame is not None:
            l_name, l_seq = np.zeros(n, np.int32), np.zeros(n, np.int32)
            self._L.csv_bam_chunk_lengths(self._h, l_name.ctypes.data if n else None, l_seq.ctypes.data if n else None)
            return FramedChunk(self, chrom, refid, _from_ptr(cc.rec_off, n, np.int64), _from_ptr(cc.rec_len, n, np.uint32), _from_ptr(cc.host_off, n + 1, np.int64),
                               l_name, l_seq, bool(cc.more), stats, int(cc.slim_bytes), int(cc.host_bytes))
        return Chunk(chrom, refid, _from_ptr(cc.slim, int(cc.slim_bytes), np.uint8), _from_ptr(cc.rec_off, n, np.int64), _from_ptr(cc.rec_len, n, np.uint32),
                     _from_ptr(cc.host, int(cc.host_bytes), np.uint8), _from_ptr(cc.host_off, n + 1, np.int64), bool(cc.more), stats)

    @staticmethod
    def _ranges(ranges):
        """ranges= of chunks / records -> None, or a Fortran-ordered int64 (k, 2) array (each column contiguous), k >= 1"""
        if ranges is None:
            return None
        r = np.asfortranarray(np.asarray(ranges, np.int64).reshape(-1, 2))
        if bool(np.any(r[:, 0] > r[:, 1])) or bool(np.any(r[1:, 0] < r[:-1, 1])):
            raise ValueError("ranges must be sorted and disjoint: start <= end <= the next start")
        return r

    def chunks(self, chrom, chunk_records=65536, start=-ALL, end=ALL, ranges=None):
        """the records of `chrom` (None: the unmapped tail) in file order, at most chunk_records per Chunk.  ranges: sorted, disjoint
        (start, end) pairs instead of start / end - every record that overlaps any of them, once, in file order"""
        flags = _abi.BAM_RESTART
        ranges = self._ranges(ranges)
        while True:
            ch = self._read(chrom, start, end, chunk_records, flags, ranges)
            if ch.n:
                yield ch
            if not ch.more:
                return
            flags = 0

    def records(self, chrom, start=-ALL, end=ALL, ranges=None):
        """one Chunk with the records of `chrom` that overlap [start, end): what fetch(chrom, start, end) yields, in its order.
        ranges: sorted, disjoint (start, end) pairs instead - the records that overlap any of them, each once, in file order"""
        return self._read(chrom, start, end, (1 << 31) - 8192, _abi.BAM_RESTART, self._ranges(ranges))

    def count(self, chrom):
        total, flags = 0, _abi.BAM_RESTART | _abi.BAM_COUNT_ONLY
        while True:
            n, more = self._read(chrom, -ALL, ALL, 1 << 30, flags)
            total += n
            if not more:
                return total
            flags = _abi.BAM_COUNT_ONLY


# ------------------------------------------------------------------------------------ BGZF inflate
def _inflate_ctx(inflate):
    """the `inflate` argument of BamFile -> None (host threads) or the Context"""
    if inflate is None or (isinstance(inflate, str) and inflate == "host"):
        return None
    if isinstance(inflate, str) or not hasattr(inflate, "_h") or not hasattr(inflate, "_check"):
        raise ValueError("inflate must be None, 'host' or an engine.Context, not %r" % (inflate,))
    return inflate


def _frame_route(frame, inflate_ctx):
    """the `frame` argument of BamFile -> "host" or "device" (which needs a device inflate route)"""
    if frame is None or (isinstance(frame, str) and frame == "host"):
        return "host"
    if not (isinstance(frame, str) and frame == "device"):
        raise ValueError("frame must be None, 'host' or 'device', not %r" % (frame,))
    if inflate_ctx is None:
        raise ValueError("frame='device' needs the device inflate route: inflate=<engine.Context>")
    return "device"


INFLATE_STATUS = dict(header=1, lengths=2, symbol=4, distance=8, output=16, short=32, input=64, crc=128)      # CSV_INF_E_*


def inflate_blocks(ctx, payloads, isizes, crcs, guard=0):
    """csv_bgzf_inflate on raw-deflate payloads -> ([bytes per block], status uint8[n], ms_kernels).  Block k's bytes are what the
    device wrote for it - exactly zlib's when status[k] == 0, unspecified otherwise.  guard: that many bytes of 0xA5 stand in front
    of and behind the output buffer, and they are returned as a fourth item (front + back) for tests of the entry's bounds."""
    n = len(payloads)
    in_len = np.array([len(p) for p in payloads], np.int32)
    in_off = np.zeros(n, np.int64)
    if n:
        in_off[1:] = np.cumsum(in_len[:-1], dtype=np.int64)
    out_len = np.asarray(isizes, np.int32).reshape(n)
    out_off = np.zeros(n, np.int64)
    if n:
        out_off[1:] = np.cumsum(out_len[:-1], dtype=np.int64)
    comp = np.frombuffer(b"".join(bytes(p) for p in payloads), np.uint8)
    total = int(out_len.sum(dtype=np.int64)) if n else 0
    buf = np.full(total + 2 * guard, 0xA5, np.uint8)
    crc = np.asarray(crcs, np.uint32).reshape(n)
    status = np.zeros(n, np.uint8)
    ms = C.c_double()
    ptr = lambda a: a.ctypes.data if len(a) else None                              # noqa: E731
    rc = lib().csv_bgzf_inflate(ctx._h, ptr(comp), len(comp), n, ptr(in_off), ptr(in_len), ptr(out_off), ptr(out_len), ptr(crc),
                                buf.ctypes.data + guard if total else None, total, 0, ptr(status), C.byref(ms))
    ctx._check(rc)
    out = buf[guard : guard + total]
    blocks = [out[int(o) : int(o) + int(ln)].tobytes() for o, ln in zip(out_off, out_len)]
    if guard:
        return blocks, status, float(ms.value), np.concatenate([buf[:guard], buf[guard + total:]])
    return blocks, status, float(ms.value)


def inflate_blocks_host(payloads, isizes, crcs):
    """the twin of inflate_blocks on zlib.decompress(p, -15) and zlib.crc32: ([bytes per block], ok bool[n]).  ok[k]: the payload
    inflates, to exactly isizes[k] bytes with CRC32 crcs[k] (an empty block is ok as it is); the checker says no more than that."""
    blocks, ok = [], np.zeros(len(payloads), bool)
    for k, (p, isize, crc) in enumerate(zip(payloads, isizes, crcs)):
        if int(isize) == 0:
            blocks.append(b""); ok[k] = True
            continue
        try:
            data = zlib.decompress(bytes(p), -15)
        except zlib.error:
            data = None
        ok[k] = data is not None and len(data) == int(isize) and (zlib.crc32(data) & 0xFFFFFFFF) == int(crc)
        blocks.append(data if ok[k] else b"")
    return blocks, ok


# ------------------------------------------------------------------------------------ decode: device
def decode(ctx, chunk, host_outputs=True):
    """csv_bam_decode on a Chunk -> dict of the columns of csv_bam_out (+ n_ops, n_sa, ms_device, ms_upload, bytes_uploaded).
    The columns also stay in the context's device memory until its next decode: extract.cigar_signatures(..., from_bam=True)
    scans them there.  host_outputs=False: only the small per-record columns come back (no CIGAR array)."""
    L = lib()
    n = chunk.n
    framed = getattr(chunk, "framed", False) and not chunk.fetched and chunk.ctx is ctx      # (on another context the images are fetched, as for the other two consumers)
    if framed:                                            # csv_bam_decode_framed takes the slim image where it lies
        chunk.check()
        slim_bytes = chunk.slim_bytes
    else:
        slim, rec_off, rec_len = np.ascontiguousarray(chunk.slim, np.uint8), np.ascontiguousarray(chunk.rec_off, np.int64), np.ascontiguousarray(chunk.rec_len, np.uint32)
        slim_bytes = len(slim)
        bin_ = BamIn(n_records=n, slim=slim.ctypes.data if len(slim) else None, slim_bytes=len(slim), rec_off=rec_off.ctypes.data if n else None,
                     rec_len=rec_len.ctypes.data if n else None)
    bound = slim_bytes // 4 + 1                           # an operation or an SA tag takes at least 4 bytes of the image
    size = dict(n=n, n1=n + 1, o=bound if host_outputs else 0, s=bound)
    arrs = {name: np.zeros(size[k], dt) if k in ("n", "n1") else np.empty(size[k], dt) for name, dt, k in _OUT}
    out = BamOut(cap_ops=size["o"], cap_sa=size["s"], **{k: (v.ctypes.data if len(v) else None) for k, v in arrs.items()})
    ctx._check(L.csv_bam_decode_framed(ctx._h, C.byref(out)) if framed else L.csv_bam_decode(ctx._h, C.byref(bin_), C.byref(out)))
    cut = dict(n=n, n1=n + 1, o=int(out.n_ops) if host_outputs else 0, s=int(out.n_sa))
    cols = {name: (arrs[name][:cut[k]].copy() if k in ("o", "s") else arrs[name]) for name, _, k in _OUT}
    cols.update(n_ops=int(out.n_ops), n_sa=int(out.n_sa), ms_device=float(out.ms_device), ms_upload=float(out.ms_upload),
                bytes_uploaded=int(out.bytes_uploaded), on_device=True)
    return cols


# ------------------------------------------------------------------------------------ decode: host
_AUX_SIZE = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
_REF_OPS = (0, 2, 3, 7, 8)                                 # M D N = X


def _aux_walk(s, p, end):
    """the tags of the aux area [p, end) of the bytes `s`: [(key, type, subtype, value begin, value end)], well-formed"""
    tags = []
    while p < end:
        if end - p < 3:
            return tags, False
        key, typ = s[p : p + 2], s[p + 2]
        p += 3
        sub = 0
        if typ in _AUX_SIZE:
            b, e = p, p + _AUX_SIZE[typ]
            if e > end:
                return tags, False
            p = e
        elif typ in (ord("Z"), ord("H")):
            q = s.find(b"\0", p, end)
            if q < 0:
                return tags, False
            b, e, p = p, q, q + 1
        elif typ == ord("B"):
            if end - p < 5:
                return tags, False
            sub = s[p]
            cnt = int.from_bytes(s[p + 1 : p + 5], "little")
            if sub not in _AUX_SIZE or sub == ord("A"):
                return tags, False
            p += 5
            if cnt > (end - p) // _AUX_SIZE[sub]:
                return tags, False
            b, e = p, p + cnt * _AUX_SIZE[sub]
            p = e
        else:
            return tags, False
        tags.append((key, typ, sub, b, e))
    return tags, True


def decode_host(chunk, check=True):
    """What csv_bam_decode computes, in numpy (fixed fields) and Python (aux walk, CIGAR): the same dict of columns.
    check: raise BamError when a record is malformed (status != 0), as the device entry fails with E_INVALID."""
    n = chunk.n
    s = chunk.slim.tobytes()
    w = chunk.slim[: len(chunk.slim) // 4 * 4].view(np.uint32)
    base = (chunk.rec_off // 4).astype(np.int64)
    fld = lambda k: w[base + k] if n else np.zeros(0, np.uint32)                   # noqa: E731
    pos = fld(1).astype(np.int32).astype(np.int64)
    flag = (fld(3) >> 16).astype(np.int32)
    cols = dict(ref_start=pos, flag=flag, mapq=((fld(2) >> 8) & 255).astype(np.int32), query_len=fld(4).astype(np.int32),
                cls=np.where((flag == 256) | (flag == 272), 0, np.where((flag == 0) | (flag == 16), 1, 2)).astype(np.uint8))
    n_cig = (fld(3) & 0xFFFF).astype(np.int64)
    l_seq = fld(4).astype(np.int64)
    ref_end, cl, cr = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    status, cg_beg, cg_end = np.zeros(n, np.uint8), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    cig_off, sa_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    cig_parts, sa_beg, sa_end = [], [], []
    for i in range(n):
        off, ln, nc = int(chunk.rec_off[i]), int(chunk.rec_len[i]), int(n_cig[i])
        if 32 + 4 * nc > ln:
            status[i] |= 2
            nc = 0
        tags, ok = _aux_walk(s, off + 32 + 4 * nc, off + ln)
        if not ok:
            status[i] |= 1
        src, n_ops = off + 32, nc
        for key, typ, sub, b, e in tags:
            if key == b"SA" and typ == ord("Z"):
                sa_beg.append(b); sa_end.append(e)
            elif key == b"CG" and typ == ord("B") and sub == ord("I") and cg_beg[i] < 0:
                cg_beg[i], cg_end[i] = b, e
        if nc == 2 and cg_beg[i] >= 0:
            op0, op1 = int(w[off // 4 + 8]), int(w[off // 4 + 9])
            if op0 & 15 == 4 and op0 >> 4 == int(l_seq[i]) and op1 & 15 == 3:
                src, n_ops = int(cg_beg[i]), int(cg_end[i] - cg_beg[i]) // 4
        ops = np.frombuffer(s, np.uint32, n_ops, src) if n_ops else np.zeros(0, np.uint32)
        cig_parts.append(ops)
        cig_off[i + 1] = cig_off[i] + n_ops
        sa_off[i + 1] = len(sa_beg)
        ref_end[i] = pos[i] + int((ops >> 4)[np.isin(ops & 15, _REF_OPS)].sum(dtype=np.int64))
        if n_ops:
            if int(ops[0]) & 15 in (4, 5):
                cl[i] = int(ops[0]) >> 4
            if int(ops[-1]) & 15 in (4, 5):
                cr[i] = int(ops[-1]) >> 4
    cols.update(ref_end=ref_end, clip_left=cl, clip_right=cr, status=status, cig_off=cig_off,
                cigar=np.concatenate(cig_parts) if cig_parts else np.zeros(0, np.uint32), sa_off=sa_off,
                sa_beg=np.asarray(sa_beg, np.int64), sa_end=np.asarray(sa_end, np.int64), cg_beg=cg_beg, cg_end=cg_end)
    cols.update(n_ops=int(cig_off[-1]), n_sa=len(sa_beg), on_device=False)
    if check and status.any():
        raise BamError("%d record(s) of the chunk have a malformed aux area or CIGAR (first: record %d)" % (int((status != 0).sum()), int(np.flatnonzero(status)[0])))
    return cols


COLUMNS = tuple(name for name, _, _ in _OUT)


# ------------------------------------------------------------------------------------ coordinate sort
SORT_ROUTES = ("device", "host")
_SORT_COUNTS = ("records", "inversions", "inflated_bytes", "stream_bytes", "out_bytes", "blocks", "slices", "passes", "bytes_up", "bytes_down")


def sort_bam(path, out, ctx=None, route="device", inflate=None, frame=None, threads=None, max_bytes=None, slice_blocks=None, index=False, overwrite=False,
             window_blocks=None):
    """Sort the BAM file `path` by coordinate into `out`: the job of samtools sort, and with index= of
    samtools sort --write-index.  The file is opened here, and only here is a header that does not say SO:coordinate accepted.
    route "device": csv_bam_sort on `ctx` (None: a Context on device 0 for the call) - keys, order, gather and compression on the
    device; "host": csv_bam_sort_host, the same rules on the host and the same file byte for byte.  inflate / frame / threads /
    window_blocks pick the reader's routes as BamFile does; inflate="device" means `ctx`.  max_bytes: the budget for the inflated
    stream plus one slice (None: half of the device's free memory; no limit on the host route); a file beyond it raises BamError
    before anything is read.  slice_blocks: BGZF blocks of 65280 bytes per slice (None: 256).  index: False, "bai" (or True) or
    "csi" - BamFile(out).build_index(write=True) on the written file, on the same routes.
    A SAM input (plain text, told by content: sam.is_sam) is converted first - sam.sam_to_bam on the same `route`, into a temporary BAM
    beside `out` that is removed at the end - and stats["sam"] holds that conversion's stats.
    The file is written through a temporary file beside `out` and os.replace.  FileExistsError, before anything is read, when `out`
    exists and overwrite is not set.  BamError "cannot sort: record N ...": a refID the header does not have or a pos below -1; nothing
    is written.  -> stats: records, inversions (0: the input was in order), inflated_bytes, stream_bytes, out_bytes, blocks, slices,
    passes, bytes_up, bytes_down, ms (wall), ms_keys / ms_sort / ms_gather / ms_deflate (device time), route, inflate, frame,
    block_table (uoff, coff, isize) and - with index= - index, the stats of the index build."""
    if route not in SORT_ROUTES:
        raise ValueError("route must be one of %s, not %r" % (", ".join(SORT_ROUTES), route))
    if index not in (False, None, True, "bai", "csi"):
        raise ValueError("index is False, \"bai\" or \"csi\", not %r" % (index,))
    out = os.fspath(out)
    if os.path.exists(out) and not overwrite:
        raise FileExistsError("%s exists (overwrite=True replaces it)" % out)
    if os.path.exists(out) and os.path.samefile(path, out):
        raise ValueError("%s cannot be sorted onto itself" % out)
    own = None
    wants_ctx = route == "device" or (isinstance(inflate, str) and inflate == "device")
    if wants_ctx and ctx is None:
        from . import engine
        own = ctx = engine.Context(0)
    from . import sam as sam_mod
    if sam_mod.is_sam(path):
        # SAM text: converted on the sort's route into a temporary BAM beside `out`, which is then sorted as any other
        fd, converted = tempfile.mkstemp(prefix=os.path.basename(out) + ".", suffix=".sam.bam", dir=os.path.dirname(out) or ".")
        os.close(fd)
        try:
            sam_stats = sam_mod.sam_to_bam(path, converted, ctx=ctx, route=route, threads=threads, overwrite=True)
            stats = sort_bam(converted, out, ctx=ctx, route=route, inflate=inflate, frame=frame, threads=threads, max_bytes=max_bytes, slice_blocks=slice_blocks, index=index,
                             overwrite=overwrite, window_blocks=window_blocks)
            stats["sam"] = sam_stats
            return stats
        finally:
            if os.path.exists(converted):
                os.unlink(converted)
            if own is not None:
                own.close()
    if isinstance(inflate, str) and inflate == "device":
        inflate = ctx
    if route == "host" and not (frame is None or frame == "host"):
        raise ValueError("route='host' frames on the host")
    tmp = None
    try:
        bf = BamFile(path, threads=threads, inflate=inflate, index=False, frame=None, _any_order=True)
        try:
            if window_blocks is not None:
                bf.set_inflate(inflate, window_blocks=window_blocks)
            bf.set_frame(frame)
            fd, tmp = tempfile.mkstemp(prefix=os.path.basename(out) + ".", suffix=".tmp", dir=os.path.dirname(out) or ".")
            os.close(fd)
            os.unlink(tmp)                                     # (the library creates the file itself, and only after the verdict)
            bf._read_serial += 1
            t0 = time.perf_counter()
            budget = 0 if max_bytes is None else int(max_bytes)
            if max_bytes is not None and budget <= 0:
                raise ValueError("max_bytes must be positive, not %r" % (max_bytes,))
            blocks = 0 if slice_blocks is None else int(slice_blocks)
            if slice_blocks is not None and not 1 <= blocks <= 32768:
                raise ValueError("slice_blocks must lie in 1 .. 32768, not %r" % (slice_blocks,))
            if route == "device":
                rc = bf._L.csv_bam_sort(bf._h, ctx._h, os.fsencode(tmp), budget, blocks, 0)
            else:
                rc = bf._L.csv_bam_sort_host(bf._h, os.fsencode(tmp), budget, blocks, 0)
            ms = (time.perf_counter() - t0) * 1e3
            if rc:
                raise BamError("%s: %s" % (path, bf._error_text()))
            counts, dev_ms = np.zeros(len(_SORT_COUNTS), np.int64), np.zeros(4, np.float64)
            bf._L.csv_bam_sort_stats(bf._h, counts.ctypes.data, dev_ms.ctypes.data)
            stats = dict(zip(_SORT_COUNTS, (int(v) for v in counts)))
            stats.update(ms=ms, ms_keys=float(dev_ms[0]), ms_sort=float(dev_ms[1]), ms_gather=float(dev_ms[2]), ms_deflate=float(dev_ms[3]), route=route,
                         inflate="host" if bf.inflate is None else "device", frame="host" if bf.frame is None else "device", written=out, index=None)
            nb = stats["blocks"]
            uoff, coff, isize, need = np.zeros(nb, np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.uint32), C.c_int64()
            if bf._L.csv_bam_sort_blocks(bf._h, uoff.ctypes.data, coff.ctypes.data, isize.ctypes.data, nb, C.byref(need)):
                raise BamError("%s: the block table of the sorted file cannot be fetched" % path)
            stats["block_table"] = (uoff, coff, isize)
        finally:
            bf.close()
        os.replace(tmp, out)
        tmp = None
        if index not in (False, None):
            fmt = "bai" if index is True else index
            with BamFile(out, threads=threads, inflate=inflate, frame=frame, index=False) as sf:
                stats["index"] = sf.build_index(write=True, overwrite=overwrite, format=fmt)
        return stats
    finally:
        if tmp is not None and os.path.exists(tmp):
            os.unlink(tmp)
        if own is not None:
            own.close()


def sort_bam_host_twin(path, out, **kw):
    """sort_bam on route "host": the twin of the device route - the same order, the same refusals, the same file"""
    return sort_bam(path, out, route="host", **kw)


# ------------------------------------------------------------------------------------ command line
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cutesv_amd.bam", description="header and per-contig record counts of a coordinate-sorted BAM file")
    ap.add_argument("bam", help="the BAM file; with --sort also SAM text")
    ap.add_argument("--chrom", default=None, help="only this contig")
    ap.add_argument("--threads", type=int, default=None, help="host threads of the inflate (default: min(16, CPUs))")
    ap.add_argument("--dump-columns", metavar="DIR", default=None, help="write the decoded columns of --chrom (host decode) as DIR/<column>.npy")
    ap.add_argument("--inflate", default="host", choices=["host", "device"], help="where the BGZF blocks are inflated: host threads, or the GPU (device 0) [%(default)s]")
    ap.add_argument("--frame", default="host", choices=["host", "device"], help="where the records are framed: on the host, or on the GPU (needs --inflate device) [%(default)s]")
    ap.add_argument("--idxstats", action="store_true", help="print contig, length, mapped and unmapped reads from the index (the table of samtools idxstats) and stop")
    ap.add_argument("--index", action="store_true", help="build the BAM index and write it to FILE.bai (the job of samtools index) on the routes of --inflate / --frame, and stop")
    ap.add_argument("--csi", action="store_true", help="with --index: build a CSI index and write it to FILE.csi (samtools index -c): the format for contigs of 2^29 bases or more")
    ap.add_argument("--min_shift", type=int, default=14, metavar="N", help="with --index --csi: 2^N bases per window of the index [14]")
    ap.add_argument("--index_out", metavar="PATH", default=None, help="with --index: write the index there instead")
    ap.add_argument("--force", action="store_true", help="with --index or --sort: replace a file that exists")
    ap.add_argument("--sort", action="store_true", help="sort FILE by coordinate into -o OUT (the job of samtools sort; with --index: of samtools sort --write-index), and stop")
    ap.add_argument("-o", "--output", metavar="OUT", default=None, help="with --sort: the sorted file")
    ap.add_argument("--sort_route", default="device", choices=["host", "device"], help="with --sort: where keys, order, gather and compression run [%(default)s]")
    ap.add_argument("--max_bytes", type=int, default=None, metavar="N", help="with --sort: the budget for the inflated stream plus one slice [device: half of the free memory]")
    a = ap.parse_args(argv)
    if (a.output is not None or a.sort_route != "device" or a.max_bytes is not None) and not a.sort:
        ap.error("-o, --sort_route and --max_bytes go with --sort")
    if a.sort and a.output is None:
        ap.error("--sort needs -o OUT")
    if a.sort and (a.index_out is not None or a.idxstats or a.dump_columns or a.chrom is not None):
        ap.error("--sort goes with -o, --index, --csi, --force, --sort_route, --max_bytes, --inflate, --frame and --threads only")
    if a.sort and a.sort_route == "host" and a.frame == "device":
        ap.error("--sort_route host frames on the host")
    if (a.index_out is not None or a.force) and not (a.index or a.sort):
        ap.error("--index_out goes with --index, --force with --index or --sort")
    if (a.csi or a.min_shift != 14) and not a.index:
        ap.error("--csi and --min_shift go with --index")
    if a.min_shift != 14 and not a.csi:
        ap.error("--min_shift goes with --csi")
    if a.idxstats:
        with BamFile(a.bam, threads=a.threads, index=True) as bf:
            for (name, mapped, unmapped, _), length in zip(bf.index_statistics(), bf.lengths):
                print("%s\t%d\t%d\t%d" % (name, length, mapped, unmapped))
            print("*\t0\t0\t%d" % (bf.no_coordinate or 0))
        return 0
    if a.frame == "device" and a.inflate != "device":
        ap.error("--frame device needs --inflate device")
    ctx = None
    if a.inflate == "device" or (a.sort and a.sort_route == "device"):
        from . import engine
        ctx = engine.Context(0)
    try:
        return _main(a, ap, ctx)
    finally:
        if ctx is not None:
            ctx.close()


def _main(a, ap, ctx):
    if a.sort:
        try:
            st = sort_bam(a.bam, a.output, ctx=ctx, route=a.sort_route, inflate=ctx if a.inflate == "device" else None, frame=a.frame, threads=a.threads, max_bytes=a.max_bytes,
                          index=("csi" if a.csi else "bai") if a.index else False, overwrite=a.force)
        except FileExistsError as e:
            ap.error("%s: --force replaces it" % e)
        print("wrote %s: %d records (%d adjacent inversions) in %d blocks, %d -> %d bytes, %.1f ms (sort %s, inflate %s, frame %s)"
              % (st["written"], st["records"], st["inversions"], st["blocks"], st["inflated_bytes"], st["out_bytes"], st["ms"], st["route"], st["inflate"], st["frame"]))
        if st["index"] is not None:
            print("wrote %s: %d bytes" % (st["index"]["written"], st["index"]["index_bytes"]))
        return 0
    if a.index:
        with BamFile(a.bam, threads=a.threads, inflate=ctx, frame=a.frame, index=False) as bf:
            try:
                st = bf.build_index(write=a.index_out if a.index_out is not None else True, overwrite=a.force, format="csi" if a.csi else "bai", min_shift=a.min_shift)
            except FileExistsError as e:
                ap.error("%s: --force replaces it" % e)
            print("wrote %s: %d bytes, %d records, %d chunks before joining, %.1f ms (inflate %s, frame %s)"
                  % (st["written"], st["index_bytes"], st["records"], st["runs"], st["ms"], st["inflate"], st["frame"]))
        return 0
    with BamFile(a.bam, threads=a.threads, inflate=ctx, frame=a.frame) as bf:
        print(bf.header_text.rstrip("\n"))
        names = [a.chrom] if a.chrom is not None else list(bf.references) + [None]
        for name in names:
            print("%s\t%d" % ("*" if name is None else name, bf.count(name)))
        if a.dump_columns:
            if a.chrom is None:
                ap.error("--dump-columns needs --chrom")
            os.makedirs(a.dump_columns, exist_ok=True)
            parts = [decode_host(ch, check=False) for ch in bf.chunks(a.chrom)]
            for k in COLUMNS:
                if k in ("cig_off", "sa_off"):              # offsets restart in every chunk: made global here
                    tot, pieces = 0, [np.zeros(1, np.int64)]
                    for c in parts:
                        pieces.append(c[k][1:] + tot); tot += int(c[k][-1])
                    arr = np.concatenate(pieces)
                else:
                    arr = np.concatenate([c[k] for c in parts]) if parts else np.zeros(0)
                np.save(os.path.join(a.dump_columns, k + ".npy"), arr)
            print("wrote %d columns to %s" % (len(COLUMNS), a.dump_columns))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
