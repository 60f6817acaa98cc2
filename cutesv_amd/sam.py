"""SAM text -> BAM: what `minimap2 -a` writes becomes the file `bam.sort_bam` takes, with no other tool.

    stats = sam_to_bam("reads.sam", "reads.bam")                    # the device route: csv_sam_to_bam
    stats = sam_to_bam("reads.sam", "reads.bam", route="host")      # csv_sam_to_bam_host: the same file byte for byte
    python -m cutesv_amd.sam FILE.sam -o OUT.bam [--route host|device] [--force]

The rules are csrc/sam_core.h's: the leading @ lines are the header, every alignment line one record; a line outside them is refused
by its 1-based line number and nothing is written.  Plain text only: SAM compressed with gzip or BGZF is not read here, CRAM neither."""
import ctypes as C
import os
import tempfile
import time

import numpy as np

from . import _lib

ROUTES = ("device", "host")
_COUNTS = ("lines", "records", "header_bytes", "text_bytes", "stream_bytes", "out_bytes", "blocks", "windows", "float_patches", "cg_records", "bytes_up", "bytes_down")
_QNAME = frozenset(range(33, 127)) - {ord("@")}


class SamError(ValueError):
    """a SAM file this project does not convert; the message names the file and the line"""


def is_sam(path):
    """Decides by content: the first two bytes are not the gzip magic, and the first byte is `@` or a byte a QNAME may begin with."""
    with open(path, "rb") as f:
        head = f.read(2)
    if len(head) < 1 or head == b"\x1f\x8b":
        return False
    return head[0] == ord("@") or head[0] in _QNAME


def default_threads():
    return max(1, min(16, os.cpu_count() or 1))


def sam_to_bam(path, out, ctx=None, route="device", threads=None, window_bytes=None, overwrite=False):
    """Convert the SAM file `path` into the BAM file `out`.  route "device": csv_sam_to_bam on `ctx` (None: a Context on device 0 for
    the call); "host": csv_sam_to_bam_host on `threads` host threads (None: min(16, CPUs)).  window_bytes: text per window (None: 64
    MiB); the file does not depend on it.  The file is written through a temporary name beside `out` and os.replace.  FileExistsError,
    before anything is read, when `out` exists and overwrite is not set.  SamError "line N ...": the lowest refused line; nothing is
    written.  -> stats: lines, records, header_bytes, text_bytes, stream_bytes, out_bytes, blocks, windows, float_patches, cg_records,
    bytes_up, bytes_down, ms (wall), ms_lines / ms_plan / ms_write / ms_deflate (device time), route, written."""
    if route not in ROUTES:
        raise ValueError("route must be one of %s, not %r" % (", ".join(ROUTES), route))
    out = os.fspath(out)
    if os.path.exists(out) and not overwrite:
        raise FileExistsError("%s exists (overwrite=True replaces it)" % out)
    if os.path.exists(out) and os.path.samefile(path, out):
        raise ValueError("%s cannot be converted onto itself" % out)
    wb = 0 if window_bytes is None else int(window_bytes)
    if window_bytes is not None and not 1 <= wb < (1 << 31) - 1:
        raise ValueError("window_bytes must lie in 1 .. 2^31 - 2, not %r" % (window_bytes,))
    L = _lib.lib()
    own = None
    if route == "device" and ctx is None:
        from . import engine
        own = ctx = engine.Context(0)
    tmp = None
    try:
        fd, tmp = tempfile.mkstemp(prefix=os.path.basename(out) + ".", suffix=".tmp", dir=os.path.dirname(out) or ".")
        os.close(fd)
        os.unlink(tmp)                                     # (the library creates the file itself, and only after the verdict)
        t0 = time.perf_counter()
        if route == "device":
            rc = L.csv_sam_to_bam(ctx._h, os.fsencode(path), os.fsencode(tmp), wb, 0)
            text = L.csv_last_error(ctx._h).decode("utf-8", "replace") if rc else ""
        else:
            err = C.create_string_buffer(512)
            rc = L.csv_sam_to_bam_host(os.fsencode(path), os.fsencode(tmp), wb, default_threads() if threads is None else int(threads), err, len(err))
            text = err.value.decode("utf-8", "replace")
        ms = (time.perf_counter() - t0) * 1e3
        if rc:
            raise SamError("%s: %s" % (path, text))
        counts, dev_ms = np.zeros(len(_COUNTS), np.int64), np.zeros(4, np.float64)
        L.csv_sam_stats(ctx._h if route == "device" else None, counts.ctypes.data, dev_ms.ctypes.data)
        stats = dict(zip(_COUNTS, (int(v) for v in counts)))
        stats.update(ms=ms, ms_lines=float(dev_ms[0]), ms_plan=float(dev_ms[1]), ms_write=float(dev_ms[2]), ms_deflate=float(dev_ms[3]), route=route, written=out)
        os.replace(tmp, out)
        tmp = None
        return stats
    finally:
        if tmp is not None and os.path.exists(tmp):
            os.unlink(tmp)
        if own is not None:
            own.close()


def records(text, names, first_line=1):
    """csv_sam_records: the line rule over `text` (bytes: whole alignment lines) on the host, without files -> (the records back to
    back, dict(lines, float_patches, cg_records)).  names: the reference names in header order.  SamError "line N ..." on a refusal."""
    L = _lib.lib()
    blob = b"".join(n.encode() if isinstance(n, str) else bytes(n) for n in names)
    off = np.zeros(len(names) + 1, np.int32)
    off[1:] = np.cumsum([len(n.encode() if isinstance(n, str) else n) for n in names], dtype=np.int64)
    tbuf, nbuf = np.frombuffer(text, np.uint8), np.frombuffer(blob, np.uint8)
    need, counts, err = C.c_int64(), np.zeros(3, np.int64), C.create_string_buffer(512)
    args = (tbuf.ctypes.data if len(text) else None, len(text), len(names), nbuf.ctypes.data if len(blob) else None, off.ctypes.data, int(first_line))
    rc = L.csv_sam_records(*args, None, 0, C.byref(need), counts.ctypes.data, err, len(err))
    if rc not in (0, 2):
        raise SamError(err.value.decode("utf-8", "replace"))
    out = np.zeros(max(1, need.value), np.uint8)
    rc = L.csv_sam_records(*args, out.ctypes.data, need.value, C.byref(need), counts.ctypes.data, err, len(err))
    if rc:
        raise SamError(err.value.decode("utf-8", "replace"))
    return out[: need.value].tobytes(), dict(lines=int(counts[0]), float_patches=int(counts[1]), cg_records=int(counts[2]))


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m cutesv_amd.sam", description="SAM text to BAM (the job of samtools view -b)")
    ap.add_argument("sam")
    ap.add_argument("-o", "--output", metavar="OUT", required=True, help="the BAM file")
    ap.add_argument("--route", default="device", choices=["host", "device"], help="where the records are written and compressed [%(default)s]")
    ap.add_argument("--threads", type=int, default=None, help="host threads of --route host (default: min(16, CPUs))")
    ap.add_argument("--force", action="store_true", help="replace a file that exists")
    a = ap.parse_args(argv)
    try:
        st = sam_to_bam(a.sam, a.output, route=a.route, threads=a.threads, overwrite=a.force)
    except FileExistsError as e:
        ap.error("%s: --force replaces it" % e)
    print("wrote %s: %d records in %d blocks, %d -> %d bytes, %.1f ms (route %s)" % (st["written"], st["records"], st["blocks"], st["text_bytes"], st["out_bytes"], st["ms"], st["route"]))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
