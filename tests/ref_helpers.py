"""Fixtures of tests/test_bgzf_reference.py: crafted FASTA texts, their BGZF images under chosen block cuts, and the two gather
entries (csv_ref_gather, csv_ref_gather_host) on blocks given as (uncompressed offset, bytes)."""
import ctypes as C
import struct
import zlib

import numpy as np

import bam_writer
from cutesv_amd import _abi, _lib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
TILE = 4096                              # ref_core.h's REF_TILE
LINE_BASES = (1, 2, 59, 60, 61, 63, 64, 65, 4096, 70000, None)           # None: the whole contig on one line


def bases(n, seed):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGTNacgtRY", np.uint8), n).tobytes()


def contig_text(name, seq, lb, nl=b"\n", description=b" crafted"):
    lb = lb or max(len(seq), 1)
    return b">" + name + description + nl + b"".join(seq[i:i + lb] + nl for i in range(0, len(seq), lb))


def crafted_fasta(nl=b"\n", n=300, big=True):
    """-> (text, {name: sequence}): a contig per line length of LINE_BASES (the 4096 and 70000 ones only with big), each with a
    short last line, then one whose last line is full, and a contig without sequence at the end"""
    seqs = {}
    for j, lb in enumerate(LINE_BASES):
        if lb is not None and lb >= 4096 and not big:
            continue
        length = n + 7 if lb is None or lb < 4096 else 2 * lb + 17
        seqs[("lb%s" % (lb or "all")).encode()] = (lb, bases(length, 100 + j))
    seqs[b"full"] = (60, bases(180, 99))
    seqs[b"empty"] = (60, b"")
    text = b"".join(contig_text(nm, s, lb, nl) for nm, (lb, s) in seqs.items())
    return text, {nm.decode(): s.decode() for nm, (_, s) in seqs.items()}


def cut_text(text, cut):
    """the pieces of text: every `cut` bytes (an int), or at the given offsets (a list)"""
    if isinstance(cut, int):
        return [text[i:i + cut] for i in range(0, len(text), cut)] or [b""]
    edges = [0] + sorted(set(int(c) for c in cut if 0 < c < len(text))) + [len(text)]
    return [text[a:b] for a, b in zip(edges[:-1], edges[1:])]


def bgzf_image(pieces, eof=True, level=1):
    return b"".join(bam_writer.bgzf_block(p, level=level) for p in pieces) + (EOF_BLOCK if eof else b"")


def write_pair(d, text, cut, name="ref"):
    """text as d/name.fa and, BGZF-compressed under `cut`, as d/name.fa.gz -> (plain path, compressed path, image)"""
    plain, gz = str(d / (name + ".fa")), str(d / (name + ".fa.gz"))
    image = bgzf_image(cut_text(text, cut))
    with open(plain, "wb") as f:
        f.write(text)
    with open(gz, "wb") as f:
        f.write(image)
    return plain, gz, image


# ------------------------------------------------------------------------------------ the entries on crafted blocks
class Blocks:
    """blocks [(uoff, bytes)] sorted by uoff -> the arrays both entries take; damage: {index: "crc" | "truncate"}"""

    def __init__(self, blocks, damage=None, level=1):
        self.uoff = np.array([u for u, _ in blocks], np.int64)
        self.isize = np.array([len(d) for _, d in blocks], np.int32)
        self.crc = np.array([zlib.crc32(d) & 0xFFFFFFFF for _, d in blocks], np.uint32)
        payloads = []
        for k, (_, d) in enumerate(blocks):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            p = co.compress(d) + co.flush()
            kind = (damage or {}).get(k)
            if kind == "crc":
                self.crc[k] ^= 1
            elif kind == "truncate":
                p = p[:len(p) // 2]
            payloads.append(p)
        self.in_len = np.array([len(p) for p in payloads], np.int32)
        self.in_off = np.zeros(len(blocks), np.int64)
        if len(blocks):
            self.in_off[1:] = np.cumsum(self.in_len[:-1], dtype=np.int64)
        self.comp = np.frombuffer(b"".join(payloads), np.uint8)
        self.data = np.frombuffer(b"".join(d for _, d in blocks), np.uint8)
        self.data_off = np.zeros(len(blocks), np.int64)
        if len(blocks):
            self.data_off[1:] = np.cumsum(self.isize[:-1], dtype=np.int64)


class Ranges:
    def __init__(self, base_off, lb, lw, beg, end):
        n = len(beg)
        full = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (n,)))     # noqa: E731
        self.base_off, self.lb, self.lw = full(base_off, np.int64), full(lb, np.int32), full(lw, np.int32)
        self.beg, self.end = np.ascontiguousarray(beg, np.int64), np.ascontiguousarray(end, np.int64)
        self.n = n


def _ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def gather_host(B, R, cap=None, guard=0):
    """csv_ref_gather_host -> (rc, out uint8[need or 0], out_off, need, error text, every byte of the buffer around `out`)"""
    total = int((R.end - R.beg).sum()) if R.n else 0
    cap = total if cap is None else cap
    buf = np.full(cap + 2 * guard, 0xA5, np.uint8)
    out_off, need, err = np.full(R.n + 1, -7, np.int64), C.c_int64(-7), C.create_string_buffer(512)
    rc = _lib.lib().csv_ref_gather_host(_ptr(B.data), len(B.data), len(B.uoff), _ptr(B.data_off), _ptr(B.uoff), _ptr(B.isize), R.n, _ptr(R.base_off), _ptr(R.lb), _ptr(R.lw),
                                        _ptr(R.beg), _ptr(R.end), buf.ctypes.data + guard if cap else None, cap, out_off.ctypes.data, C.byref(need), err, len(err))
    got = buf[guard:guard + need.value] if rc == _abi.OK and 0 <= need.value <= cap else buf[:0]
    return rc, got, out_off, need.value, err.value.decode(), np.concatenate([buf[:guard], buf[guard + len(got):]])


def gather_device(ctx, B, R, cap=None, guard=0, flags=0, status_fill=0x5A):
    """csv_ref_gather -> (rc, out, out_off, need, error text, every byte of the buffer around out[0, need), status, ms)"""
    total = int((R.end - R.beg).sum()) if R.n else 0
    cap = total if cap is None else cap
    buf = np.full(cap + 2 * guard, 0xA5, np.uint8)
    out_off, need = np.full(R.n + 1, -7, np.int64), C.c_int64(-7)
    status, ms = np.full(len(B.uoff), status_fill, np.uint8), (C.c_double * 2)()
    L = _lib.lib()
    rc = L.csv_ref_gather(ctx._h, _ptr(B.comp), len(B.comp), len(B.uoff), _ptr(B.in_off), _ptr(B.in_len), _ptr(B.uoff), _ptr(B.isize), _ptr(B.crc), R.n, _ptr(R.base_off),
                          _ptr(R.lb), _ptr(R.lw), _ptr(R.beg), _ptr(R.end), buf.ctypes.data + guard if cap else None, cap, out_off.ctypes.data, C.byref(need), _ptr(status), flags, ms)
    text = (L.csv_last_error(ctx._h) or b"").decode() if rc != _abi.OK else ""
    got = buf[guard:guard + need.value] if rc == _abi.OK and 0 <= need.value <= cap else buf[:0]
    return rc, got, out_off, need.value, text, np.concatenate([buf[:guard], buf[guard + len(got):]]), status, (ms[0], ms[1])


def line_layout(seq, lb, gap, uoff0=0, head=b">c\n"):
    """one contig of `seq` with lb bases per line and `gap` line-break bytes, whose text starts at uncompressed offset uoff0 ->
    (text, base_off, lw)"""
    nl = b"\n" if gap == 1 else b"\r\n"
    lb = lb or len(seq)
    text = head + b"".join(seq[i:i + lb] + nl for i in range(0, len(seq), lb))
    return text, uoff0 + len(head), lb + gap


def blocks_at(text, cut, uoff0=0):
    out, o = [], 0
    for p in cut_text(text, cut):
        out.append((uoff0 + o, p))
        o += len(p)
    return out


def range_set(n, lb, lens_small=(0, 1, 63, 64, 65, 255, 256, 257), lens_big=(TILE - 1, TILE, TILE + 1, 65535, 65536, 65537, 200001)):
    """(beg, end) over a contig of n bases: every start residue mod 64 for the short lengths, the starts around a line's first and
    last base for the long ones, and every length ending at the contig's last base"""
    beg, end = [], []
    for ln in lens_small:
        for s in range(64):
            if s + ln <= n:
                beg.append(s); end.append(s + ln)
    for ln in lens_big:
        for s in sorted({0, 1, 2, 3, 63, 64, max(lb - 1, 0), lb, 2 * lb - 1}):
            if s + ln <= n:
                beg.append(s); end.append(s + ln)
    for ln in lens_small + lens_big:
        if ln <= n:
            beg.append(n - ln); end.append(n)
    return np.array(beg, np.int64), np.array(end, np.int64)


def truth(seq, beg, end):
    a = np.frombuffer(seq, np.uint8)
    return np.concatenate([a[b:e] for b, e in zip(beg.tolist(), end.tolist())] + [np.zeros(0, np.uint8)])
