"""BGZF inflate on the GPU (csv_bgzf_inflate: cutesv_amd/csrc/inflate_core.h, the kernel at the end of bam.hip.h, stage_inflate.hip.h;
the reader's device route in bam_host.cpp).

The corpus is tests/deflate_writer.py's: streams from zlib's compressor and streams crafted bit by bit, valid and damaged.  zlib
alone pins it (the self-check below); `bam.inflate_blocks_host` - zlib.decompress and zlib.crc32 - is the twin everything is
compared with.

CPU: the corpus self-check; the decode core's host form, built as a stand-alone program with the address and undefined-behaviour
sanitizers, over the whole corpus against the twin (the bounds are proven here, before a wavefront runs the same code); the
refusals of BamFile(inflate=); csv_bam_set_inflate(bam, NULL, 0).
GPU (-m gpu): the corpus in windows of 1 .. 300 blocks with guard bytes around the output, the CRC at the lengths where the
64-lane split changes shape, whole BAM files on both routes, the entry's isolation from the decode columns and a kept rebuild,
call_bam and the command line on both routes.

A status byte has eight bits for nine reasons: block type 3 and a stored LEN/NLEN mismatch share CSV_INF_E_HEADER."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, call, cli, extract, rebuild
from cutesv_amd.columns import Params
import bam_writer
import call_helpers
import deflate_writer as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    """(entries, the twin's bytes, the twin's ok) - computed once, shared, never changed"""
    E = dw.corpus()
    data, ok = bam.inflate_blocks_host([e.payload for e in E], [e.isize for e in E], [e.crc for e in E])
    ok.setflags(write=False)
    return E, data, ok


# ------------------------------------------------------------------------------------------------ CPU
def test_the_corpus_is_pinned_by_zlib(corpus):
    """valid entries inflate with zlib to the intended bytes; damaged streams make zlib raise; the three whose damage is in ISIZE
    or the CRC inflate, and fail the comparison the trailer asks for"""
    E, data, ok = corpus
    assert 55 <= len(E) <= 80 and len({e.name for e in E}) == len(E)
    for e, d, k in zip(E, data, ok):
        if e.data is not None:
            assert zlib.decompress(e.payload, -15) == e.data and e.isize == len(e.data) and e.crc == zlib.crc32(e.data) and e.bit == 0, e.name
            assert k and d == e.data, e.name
        elif e.stream:
            with pytest.raises(zlib.error):
                zlib.decompress(e.payload, -15)
            assert not k and e.bit in dw_bits(), e.name
        else:
            got = zlib.decompress(e.payload, -15)
            assert len(got) != e.isize or zlib.crc32(got) != e.crc, e.name
            assert (e.bit == dw.E_CRC) == (len(got) == e.isize) and (e.bit == dw.E_OUTPUT) == (len(got) > e.isize), e.name
            assert not k and e.bit in (dw.E_OUTPUT, dw.E_SHORT, dw.E_CRC), e.name
    # every status bit has its damaged entry; the kinds of blocks zlib was asked for are the kinds it gave
    assert {e.bit for e in E if e.data is None} == set(dw_bits())
    kinds = {e.name: block_types(e.payload) for e in E if e.name.startswith("zlib")}
    assert kinds["zlib level 0: stored"] == [0] and kinds["zlib Z_FIXED"] == [1] and kinds["zlib level 6: dynamic"] == [2]
    assert kinds["zlib level 0, 65536 random bytes: two stored blocks"] == [0, 0]
    assert len(kinds["zlib memLevel 1: several dynamic blocks"]) > 3
    assert 0 in kinds["zlib Z_FULL_FLUSH in mid-stream"][1:]
    assert INFLATE_BITS_MATCH


def dw_bits():
    return (dw.E_HEADER, dw.E_LENGTHS, dw.E_SYMBOL, dw.E_DISTANCE, dw.E_OUTPUT, dw.E_SHORT, dw.E_INPUT, dw.E_CRC)


INFLATE_BITS_MATCH = tuple(bam.INFLATE_STATUS[k] for k in ("header", "lengths", "symbol", "distance", "output", "short", "input", "crc")) == dw_bits()


def block_types(payload):
    """the BTYPE of every deflate block of a valid stream: a walk with the test-side tables (deflate_writer's), no output kept"""
    bits = BitReader(payload)
    out = []
    while True:
        last, typ = bits.take(1), bits.take(2)
        out.append(typ)
        if typ == 0:
            bits.align()
            n = bits.take(16); bits.take(16)
            bits.skip_bytes(n)
        else:
            if typ == 1:
                ll, d = dw.FIXED_LL, dw.FIXED_D
            else:
                nl, nd, nc = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for s in dw.CL_ORDER[:nc]:
                    cl[s] = bits.take(3)
                cc = dw.canonical(cl)
                lens = []
                while len(lens) < nl + nd:
                    s = bits.symbol(cc)
                    lens += [s] if s < 16 else [lens[-1]] * (3 + bits.take(2)) if s == 16 else [0] * (3 + bits.take(3)) if s == 17 else [0] * (11 + bits.take(7))
                ll, d = dw.canonical(lens[:nl]), dw.canonical(lens[nl:])
            while True:
                s = bits.symbol(ll)
                if s == 256:
                    break
                if s > 256:
                    bits.take(dw.LEN_TAB[s - 257][1])
                    bits.take(dw.DIST_TAB[bits.symbol(d)][1])
        if last:
            return out


class BitReader:
    def __init__(self, data):
        self.v, self.pos = int.from_bytes(data, "little"), 0

    def take(self, n):
        x = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return x

    def align(self):
        self.pos = (self.pos + 7) // 8 * 8

    def skip_bytes(self, n):
        self.pos += 8 * n

    def symbol(self, codes):
        inv = getattr(self, "_inv", {}).get(id(codes))
        if inv is None:
            inv = {(c, ln): s for s, (c, ln) in codes.items()}
            self.__dict__.setdefault("_inv", {})[id(codes)] = inv
        code = 0
        for ln in range(1, 16):
            code = code << 1 | self.take(1)
            if (code, ln) in inv:
                return inv[(code, ln)]
        raise ValueError("no code")


def test_the_decode_core_under_the_sanitizers_equals_the_twin(corpus, tmp_path):
    """inflate_core.h's host form - the code the wavefronts run, with one lane - over the whole corpus, damaged streams included, in a
    stand-alone program built with -fsanitize=address,undefined: every payload and every output is a heap block of exactly its
    size there, so a read behind a payload or a write behind out_len ends the program.  The sanitizers' runtimes are linked into it."""
    E, data, ok = corpus
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (the library's own build needs it too)"
    exe, path = str(tmp_path / "inflate_core_main"), str(tmp_path / "corpus.bin")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(ROOT, "tests", "inflate_core_main.cpp")], check=True, capture_output=True, text=True)
    dw.write_corpus(path, E)
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(len(E)))
    for e, d, k, (_, st, crc, adler) in zip(E, data, ok, rows):
        print("%-70s status %3d twin %s" % (e.name, st, "ok" if k else "not ok"))
        assert (st == 0) == bool(k), e.name
        assert st == e.bit, e.name
        if k:
            assert crc == zlib.crc32(d) and adler == zlib.adler32(d), e.name


def _small_bam(path, **kw):
    recs, _ = call_helpers.planted_records()
    return bam_writer.write_bam(path, call_helpers.CONTIGS, recs, **kw)


def _images(bf, chrom, **kw):
    out = []
    for ch in bf.chunks(chrom, **kw):
        out.append((ch.slim.tobytes(), ch.rec_off.tobytes(), ch.rec_len.tobytes(), ch.host.tobytes(), ch.host_off.tobytes(), ch.more))
    return out


def test_bamfile_refuses_an_inflate_that_is_no_route(tmp_path):
    path = str(tmp_path / "a.bam")
    _small_bam(path)
    for bad in ("device", "gpu", 0, 1.5, object()):
        with pytest.raises(ValueError, match="inflate"):
            bam.BamFile(path, inflate=bad)
    for good in (None, "host"):
        with bam.BamFile(path, inflate=good) as bf:
            assert bf.inflate is None
            ch = bf.records("chrA", 0, 1 << 40)
            assert ch.stats["inflate"] == "host" and ch.stats["device_blocks"] == 0 and ch.stats["fallback_blocks"] == 0 and ch.stats["ms_inflate_kernels"] == 0.0
            with pytest.raises(ValueError, match="inflate"):
                bf.set_inflate("device")
            for w in (-1, 16385):
                with pytest.raises(ValueError, match="window_blocks"):
                    bf.set_inflate(None, window_blocks=w)
    with pytest.raises(ValueError, match="inflate"):
        call.call_bam(path, {}, call.CallParams(Params()), inflate="gpu")
    own, rest = cli.split_own(["a", "--inflate", "device", "b", "c", "d", "-t", "2"])
    assert own.inflate == "device" and rest == ["a", "b", "c", "d", "-t", "2"]
    assert cli.split_own(["a", "b", "c", "d"])[0].inflate is None and call.DEFAULT_INFLATE in ("host", "device")


def test_set_inflate_null_is_the_host_route(tmp_path):
    """csv_bam_set_inflate(bam, NULL, 0): the host threads, the same chunk images as a reader that was never told anything"""
    path = str(tmp_path / "a.bam")
    _small_bam(path, block_bytes=3000)
    L = _lib.lib()
    with bam.BamFile(path, threads=2) as bf:
        want = {c: _images(bf, c, chunk_records=7) for c in ("chrA", "chrB")}
    assert sum(len(v) for v in want.values()) > 5
    with bam.BamFile(path, threads=2) as bf:
        assert L.csv_bam_set_inflate(bf._h, None, 0) == _abi.OK
        assert {c: _images(bf, c, chunk_records=7) for c in ("chrA", "chrB")} == want
        assert L.csv_bam_set_inflate(bf._h, None, 16385) == _abi.E_INVALID and L.csv_bam_set_inflate(None, None, 0) == _abi.E_INVALID
        dev, fb, ms = C.c_int64(-1), C.c_int64(-1), C.c_double(-1)
        assert L.csv_bam_inflate_stats(bf._h, C.byref(dev), C.byref(fb), C.byref(ms)) == _abi.OK
        assert (dev.value, fb.value, ms.value) == (0, 0, 0.0)
        assert bf.set_inflate("host") is None and {c: _images(bf, c, chunk_records=7) for c in ("chrA", "chrB")} == want


# ------------------------------------------------------------------------------------------------ GPU 1: the corpus
WINDOWS = (1, 2, 63, 64, 65, 300)


def _window(E, n, shift):
    """n blocks: corpus entries in turn from `shift` on, an empty block (out_len == 0) behind every fifth"""
    out, k = [], shift
    while len(out) < n:
        out.append(k % len(E)); k += 1
        if len(out) % 5 == 4 and len(out) < n:
            out.append(-1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_blocks", WINDOWS)
def test_gpu_corpus_equals_the_twin(ctx, corpus, n_blocks):
    E, data, ok = corpus
    # the window of 300 starts at entry 0 and holds every entry several times; the small ones start where the damaged entries are
    pick = _window(E, n_blocks, 0 if n_blocks >= len(E) else len(E) - 16 - n_blocks // 2)
    payloads = [E[i].payload if i >= 0 else b"" for i in pick]
    isizes = [E[i].isize if i >= 0 else 0 for i in pick]
    crcs = [E[i].crc if i >= 0 else 0 for i in pick]
    got, status, ms, guard = bam.inflate_blocks(ctx, payloads, isizes, crcs, guard=64)
    assert (guard == 0xA5).all() and len(guard) == 128, "bytes in front of or behind `out` were written"
    assert ms > 0 or all(s == 0 for s in isizes)
    for i, g, st in zip(pick, got, status.tolist()):
        if i < 0:
            assert st == 0 and g == b""
            continue
        e = E[i]
        print("%-70s status %3d" % (e.name, st))
        assert (st == 0) == bool(ok[i]), e.name
        assert st == e.bit, e.name                              # a valid entry: 0; a damaged one: the one bit named for it
        if ok[i]:
            assert g == data[i], e.name
    if n_blocks >= len(E):
        assert {i for i in pick if i >= 0} == set(range(len(E)))


@pytest.mark.gpu
def test_gpu_refuses_malformed_calls_and_writes_nothing(ctx, corpus):
    from cutesv_amd.engine import CsvError
    E, data, ok = corpus
    e = next(x for x in E if x.name == "zlib Z_FIXED")
    L = _lib.lib()
    comp = np.frombuffer(e.payload * 2, np.uint8)
    n = len(e.payload)

    def run(in_off, in_len, out_off, out_len, n_blocks=2, out_bytes=None, comp_bytes=None, flags=0):
        a = [np.asarray(x, dt) for x, dt in ((in_off, np.int64), (in_len, np.int32), (out_off, np.int64), (out_len, np.int32), ([e.crc, e.crc], np.uint32))]
        out = np.full(2 * e.isize + 128, 0xA5, np.uint8)
        status = np.full(2, 0xEE, np.uint8)
        rc = L.csv_bgzf_inflate(ctx._h, comp.ctypes.data, len(comp) if comp_bytes is None else comp_bytes, n_blocks, *[x.ctypes.data for x in a], out.ctypes.data + 64,
                                2 * e.isize if out_bytes is None else out_bytes, flags, status.ctypes.data, None)
        return rc, out, status
    rc, out, status = run([0, n], [n, n], [0, e.isize], [e.isize, e.isize])
    assert rc == _abi.OK and status.tolist() == [0, 0] and out[64 : 64 + 2 * e.isize].tobytes() == e.data * 2
    bad = dict(payload_outside=([0, n + 1], [n, n], [0, e.isize], [e.isize, e.isize]), negative_in_off=([-1, n], [n, n], [0, e.isize], [e.isize, e.isize]),
               negative_in_len=([0, n], [n, -1], [0, e.isize], [e.isize, e.isize]), output_outside=([0, n], [n, n], [0, e.isize + 1], [e.isize, e.isize]),
               overlap=([0, n], [n, n], [0, e.isize - 1], [e.isize, e.isize]), overlap_unsorted=([0, n], [n, n], [e.isize - 1, 0], [e.isize, e.isize]),
               too_long=([0, n], [n, n], [0, 0], [65537, 0]), negative_out_len=([0, n], [n, n], [0, e.isize], [e.isize, -1]))
    for name, args in bad.items():
        rc, out, status = run(*args, out_bytes=70000 if name == "too_long" else None)
        assert rc == _abi.E_INVALID, name
        assert (out == 0xA5).all() and (status == 0xEE).all(), name
    assert run([0, n], [n, n], [0, e.isize], [e.isize, e.isize], n_blocks=-1)[0] == _abi.E_INVALID
    assert run([0, n], [n, n], [0, e.isize], [e.isize, e.isize], flags=1)[0] == _abi.E_INVALID
    assert run([0, n], [n, n], [0, e.isize], [e.isize, e.isize], n_blocks=0)[0] == _abi.OK
    # outputs in any order, with a gap between them that stays as it was
    rc, out, status = run([0, n], [n, n], [e.isize + 7, 0], [e.isize, e.isize], out_bytes=2 * e.isize + 7)
    assert rc == _abi.OK and status.tolist() == [0, 0]
    assert out[64 : 64 + e.isize].tobytes() == e.data and out[64 + e.isize + 7 : 64 + 2 * e.isize + 7].tobytes() == e.data
    assert (out[64 + e.isize : 64 + e.isize + 7] == 0xA5).all() and (out[:64] == 0xA5).all() and (out[64 + 2 * e.isize + 7 :] == 0xA5).all()
    with pytest.raises(CsvError):
        bam.inflate_blocks(ctx, [e.payload], [65537], [e.crc])


# ------------------------------------------------------------------------------------------------ GPU 2: the CRC
CRC_LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536)


@pytest.mark.gpu
def test_gpu_crc_at_the_lengths_where_the_lanes_split_differently(ctx):
    """stored blocks of random bytes (the decode is a copy: what is tested is the CRC): status 0 with zlib.crc32, the CRC bit and
    nothing else with any other value - the kernel computes the CRC, it does not wave it through"""
    rng = np.random.default_rng(11)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in CRC_LENGTHS]
    payloads = []
    for d in datas:
        co = zlib.compressobj(0, zlib.DEFLATED, -15)
        payloads.append(co.compress(d) + co.flush())
    good = [zlib.crc32(d) for d in datas]
    wrong = [c ^ (1 << (k % 32)) for k, c in enumerate(good)]
    got, status, _ = bam.inflate_blocks(ctx, payloads * 2, [len(d) for d in datas] * 2, good + wrong)
    assert status.tolist() == [0] * len(datas) + [dw.E_CRC] * len(datas)
    assert got[: len(datas)] == datas
    # and compressed text of the same lengths (level 6: matches, several lanes' pieces written by matches)
    text = (b"GATTACA" * 10000)[:65536]
    datas = [text[:n] for n in CRC_LENGTHS]
    payloads = [dw._z(d, 6) for d in datas]
    got, status, _ = bam.inflate_blocks(ctx, payloads, [len(d) for d in datas], [zlib.crc32(d) for d in datas])
    assert status.tolist() == [0] * len(datas) and got == datas


# ------------------------------------------------------------------------------------------------ GPU 3: files
def _file_variants():
    """(records, refs, region contig) of test_bam_reader.py's cases: a golden single_pipe case and the edge records"""
    import test_bam_reader as tbr
    from helpers import load_json
    case = load_json("single_pipe.json.gz")[0]
    refs, recs = tbr.golden_records(case, "7")
    return tbr, refs, recs


def _both_routes(ctx, path, chrom, window_blocks=0):
    with bam.BamFile(path, threads=2) as bf:
        want = (_images(bf, chrom, chunk_records=50), _images(bf, chrom))
        rec = bf.records(chrom, 0, 1 << 40)
        want_rec = (rec.slim.tobytes(), rec.host.tobytes(), rec.rec_off.tobytes())
    with bam.BamFile(path, threads=2, inflate=ctx) as bf:
        if window_blocks:
            bf.set_inflate(ctx, window_blocks=window_blocks)
        got = (_images(bf, chrom, chunk_records=50), _images(bf, chrom))
        bf.set_inflate(ctx)                                     # (a window that holds the whole file would serve the next read as it is: setting the route empties it)
        rec = bf.records(chrom, 0, 1 << 40)
        st = rec.stats
        assert st["inflate"] == "device" and st["fallback_blocks"] == 0 and st["device_blocks"] > 0 and st["ms_inflate_kernels"] > 0, st
        assert (rec.slim.tobytes(), rec.host.tobytes(), rec.rec_off.tobytes()) == want_rec
    assert got == want
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("level", (0, 1, 6, 9))
def test_gpu_files_read_the_same_on_both_routes(ctx, tmp_path, level):
    tbr, refs, recs = _file_variants()
    info = bam_writer.write_bam(str(tmp_path / "base.bam"), refs, recs, level=level)
    r5, r9, r11 = info["records"][5], info["records"][9], info["records"][11]
    inside = [r5["offset"] + 2, r5["fixed"] + 13, r9["cigar"] + 6, r11["aux"] + 5, r11["aux"] + 6, info["header_end"] - 3, 9]
    small = list(range(1000, info["records"][-1]["end"], 1777))
    n = 0
    for cuts in (None, "record", inside, small):
        for block_bytes in (700, bam_writer.MAX_BLOCK):
            path = str(tmp_path / ("f%d.bam" % n))
            n += 1
            w = bam_writer.write_bam(path, refs, recs, cuts=cuts, block_bytes=block_bytes, level=level)
            st = _both_routes(ctx, path, "7", window_blocks=(0, 64, 1)[n % 3])
            assert w["n_blocks"] > 10 and st["device_blocks"] >= 10
    # the edge records: a 70 000-operation CG array cut inside, the longest name
    path = str(tmp_path / "edge.bam")
    _, info = tbr.write_edge(path, level=level)
    _both_routes(ctx, path, "7")
    r6 = info["records"][6]
    tbr.write_edge(path, cuts=[r6["aux"] + 11, r6["aux"] + 100001, r6["end"] - 1, r6["offset"] + 3], level=level, block_bytes=bam_writer.MAX_BLOCK)
    _both_routes(ctx, path, "7")


def _bgzf_blocks(blob):
    """[(offset, size)] of the BGZF blocks of a file"""
    out, o = [], 0
    while o < len(blob):
        size = struct.unpack_from("<H", blob, o + 16)[0] + 1
        out.append((o, size))
        o += size
    return out


@pytest.mark.gpu
def test_gpu_a_damaged_block_raises_the_same_on_both_routes(ctx, tmp_path):
    """one flipped payload byte in a block behind the 256 the reader inflates when it opens the file: both routes raise the same text,
    and the device route shows the one block the host had to look at again"""
    _, refs, recs = _file_variants()
    path = str(tmp_path / "many.bam")
    bam_writer.write_bam(path, refs, recs, cuts="record")
    blob = bytearray(open(path, "rb").read())
    blocks = _bgzf_blocks(blob)
    assert len(blocks) > 300
    off, size = blocks[280]
    blob[off + 18 + (size - 26) // 2] ^= 0x10
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(blob))
    texts = []
    for route in (None, ctx):
        with bam.BamFile(bad, threads=2, inflate=route) as bf:
            with pytest.raises(bam.BamError) as ei:
                bf.records("7", 0, 1 << 40)
            texts.append(str(ei.value))
            st = bf.inflate_stats()
    assert texts[0] == texts[1] and "byte %d does not inflate" % off in texts[0]
    assert st["inflate"] == "device" and st["fallback_blocks"] == 1 and st["device_blocks"] > 0
    # the undamaged file on the device route: no block falls back
    with bam.BamFile(path, inflate=ctx) as bf:
        assert bf.records("7", 0, 1 << 40).stats["fallback_blocks"] == 0


# ------------------------------------------------------------------------------------------------ GPU 4: isolation
@pytest.mark.gpu
def test_gpu_inflate_leaves_the_decode_columns_and_a_kept_rebuild_alone(ctx, corpus, tmp_path):
    import test_bam_reader as tbr
    import test_call_bam as tcb
    E, data, ok = corpus
    path = str(tmp_path / "edge.bam")
    tbr.write_edge(path)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    use = np.ones(ch.n, np.uint8)
    keys = ("ins_read", "ins_pos", "ins_len", "ins_piece0", "ins_npiece", "piece_qoff", "piece_len", "del_read", "del_pos", "del_len")

    def blocks():
        got, status, _ = bam.inflate_blocks(ctx, [e.payload for e in E], [e.isize for e in E], [e.crc for e in E])
        assert [int(s) for s in status] == [e.bit for e in E]
    cols = bam.decode(ctx, ch)
    want = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
    cols = bam.decode(ctx, ch)
    blocks()
    got = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
    assert want["n_sig_ins"] > 100
    for k in keys:
        assert np.array_equal(got[k], want[k]), k
    # a kept rebuild still answers after an inflate
    seqs, rb = tcb.alt_pool(ctx)
    src = rb["src_row"]
    ins_rows = np.flatnonzero(src < len(tcb.ALT_LENS))
    clip = np.asarray([len(seqs[int(src[r])]) for r in ins_rows], np.int64)
    want = rebuild.alt_gather_host(seqs, src, ins_rows, clip)
    blocks()
    got = rebuild.alt_gather(ctx, ins_rows, clip)
    assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and len(want[0]) > 1000
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU 5: call_bam, the command lines
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_call")
    path = str(d / "planted.bam")
    ref = call_helpers.write_planted_bam(path)
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return path, ref, fa


@pytest.mark.gpu
@pytest.mark.parametrize("genotype", (False, True))
def test_gpu_call_bam_gives_the_same_text_on_both_routes(ctx, planted, genotype, tmp_path):
    path, ref, fa = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=genotype))
    kw = dict(tra_gt="alignments" if genotype else None, report_readid=True)
    th, td = {}, {}
    host, svid_h = call.call_bam(path, ref, cp, ctx=ctx, inflate="host", timings=th, sigs_dir=str(tmp_path), **kw)
    sigs_h = {t: open(str(tmp_path / (t + ".sigs")), "rb").read() for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    dev, svid_d = call.call_bam(path, ref, cp, ctx=ctx, inflate="device", timings=td, sigs_dir=str(tmp_path), **kw)
    sigs_d = {t: open(str(tmp_path / (t + ".sigs")), "rb").read() for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    assert host.count("\n") >= 5 and "SVTYPE=INS" in host and "SVTYPE=BND" in host
    assert dev == host and svid_d.tolist() == svid_h.tolist() and sigs_d == sigs_h and len(sigs_h["INS"]) > 1000
    assert th["ms_inflate"] > 0 and td["ms_inflate"] > 0
    # a reader that was handed in inflates on the call's context during the call and has its own setting back afterwards
    with bam.BamFile(path) as bf:
        seen, read = [], bf._read
        bf._read = lambda *a, **k: (read(*a, **k), seen.append(dict(bf.last_stats)))[0]          # the stats of every read of the call
        assert call.call_bam(bf, ref, cp, ctx=ctx, inflate="device", **kw)[0] == host
        assert bf.inflate is None and len(seen) >= 2 and all(s["inflate"] == "device" and s["fallback_blocks"] == 0 for s in seen)
        assert sum(s["device_blocks"] for s in seen) > 0 and sum(s["ms_inflate_kernels"] for s in seen) > 0
        assert call.call_bam(bf, ref, cp, ctx=ctx, **kw)[0] == host
        assert bf.last_stats["inflate"] == call.DEFAULT_INFLATE
    with bam.BamFile(path, inflate=ctx) as bf:
        assert call.call_bam(bf, ref, cp, ctx=ctx, inflate="host", **kw)[0] == host
        assert bf.inflate is ctx and bf.last_stats["inflate"] == "host"


@pytest.mark.gpu
def test_gpu_command_lines_take_inflate(planted, tmp_path, capsys):
    path, ref, fa = planted
    wd = str(tmp_path / "work")
    os.mkdir(wd)
    outs = {}
    for route in ("host", "device"):
        out = str(tmp_path / (route + ".vcf"))
        assert cli.main([path, fa, out, wd, "-s", "3", "--genotype", "--inflate", route]) == 0
        data = open(out, "rb").read()
        lines = data.split(b"\n")
        outs[route] = [ln for ln in lines if not ln.startswith(b"##fileDate=") and not ln.startswith(b"##CommandLine=")]
        body = str(tmp_path / (route + ".body.vcf"))
        assert call.main([path, fa, "-o", body, "--preset", "ont", "--min_support", "3", "--inflate", route]) == 0
        outs[route + " body"] = open(body, "rb").read()
    assert outs["host"] == outs["device"] and len(outs["host"]) > 20
    assert outs["host body"] == outs["device body"] and outs["host body"].count(b"\n") >= 5
    # the counting pass
    capsys.readouterr()
    assert bam.main([path, "--inflate", "device"]) == 0
    dev = capsys.readouterr().out
    assert bam.main([path]) == 0
    assert capsys.readouterr().out == dev and "chrA\t" in dev
