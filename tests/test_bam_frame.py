"""BAM record framing on the device: frame_core.h under the sanitizers against a naive chain walk, the
fallback counts of the twin, the Python surface - and on the GPU the device chunks against the host-framing chunks of the same
file, byte for byte: block cuts at every part of a record, windows of 1, 2 and 64 blocks, decoys, damaged files, the framed
consumers, call_bam and the command lines."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, call, cli, extract, rebuild
from cutesv_amd.columns import Params
import bam_writer
import call_helpers
import frame_helpers as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("csv_bam_set_frame", "csv_bam_chunk_lengths", "csv_bam_chunk_fetch", "csv_bam_frame_stats", "csv_bam_decode_framed", "csv_name_pool_append_framed",
               "csv_seq_reads_framed")


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """frame_core_main built with the sanitizers (their runtimes linked in, nothing preloaded) -> run(windows, n_ref) -> rows of ints"""
    d = tmp_path_factory.mktemp("frame_core")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/frame_core_main.cpp")
    exe = str(d / "frame_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "frame_core_main.cpp")], check=True, capture_output=True, text=True)
    count = [0]

    def run(windows, n_ref):
        path = str(d / ("corpus%d.bin" % count[0]))
        count[0] += 1
        fh.write_corpus(path, windows, n_ref)
        p = subprocess.run([exe, path], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        rows = [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]
        assert [r[0] for r in rows] == list(range(len(windows)))
        return rows
    return run


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return fh.plain_files(tmp_path_factory.mktemp("frame_plain"))


# ------------------------------------------------------------------------------------------------ CPU 1: the core
def test_the_core_under_the_sanitizers_equals_the_naive_walk(twin, plain, tmp_path):
    rng = np.random.default_rng(29)
    windows = []
    for path, wb in plain[:6]:
        stream, lens = fh.stream_of(path)
        windows += fh.windows_of(stream, lens, wb or 4096)
    n_valid = len(windows)
    # windows of random bytes: whatever the guess chases there, it reads nothing outside and the stitch gives the naive walk
    for n in (0, 1, 3, 35, 36, 37, 100, 4096, 70000):
        for _ in range(3):
            w = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            cut = sorted(set(int(x) for x in rng.integers(0, n + 1, 4))) if n else []
            lens = [b - a for a, b in zip([0] + cut, cut + [n])]
            windows.append((w, lens, int(rng.integers(0, n + 1))))
    # random bytes in which small numbers are frequent: block_size words that lead somewhere
    for _ in range(6):
        w = np.where(rng.random(3000) < 0.7, 0, rng.integers(0, 256, 3000)).astype(np.uint8)
        w[::40] = 36
        windows.append((w.tobytes(), [1000, 0, 1500, 500], int(rng.integers(0, 80))))
    # mutated valid windows: flipped bytes anywhere - block_size words, field lengths, names
    stream, lens = fh.stream_of(plain[2][0])
    base = fh.windows_of(stream, lens, 4096)[0]
    for k in range(40):
        w = bytearray(base[0])
        for pos in rng.integers(base[2], len(w), 1 + k % 5):
            w[int(pos)] ^= int(rng.integers(1, 256))
        windows.append((bytes(w), base[1], base[2]))
    # a window cut short inside a record, inside a block_size word, and right behind one
    for cut in (1, 2, 3, 4, 5, 40):
        w = base[0][: len(base[0]) - cut]
        lens, over = list(base[1]), cut
        for k in range(len(lens) - 1, -1, -1):
            take = min(lens[k], over)
            lens[k] -= take; over -= take
        windows.append((w, lens, base[2]))
    rows = twin(windows, 2)
    for (w, lens, c), r in zip(windows, rows):
        starts, tail = fh.naive_walk(w, c)
        assert (r[1], r[2]) == (len(starts), tail), r
        assert r[7] == fh.rows_hash(w, starts), r                              # every row: the fields and the CIGAR span
    assert sum(r[1] for r in rows[:n_valid]) >= 6 * 300


def test_the_twin_counts_no_fallback_without_a_decoy(twin, plain, tmp_path):
    """the condition the GPU tests lean on: on every plain file they read, every block the chain lands in was guessed right; on the
    decoy file exactly the planted blocks are chased again"""
    for path, wb in plain:
        stream, lens = fh.stream_of(path)
        for blocks in sorted({wb or 4096, 4096}):
            rows = twin(fh.windows_of(stream, lens, blocks), 2)
            assert sum(r[6] for r in rows) == 0, (path, blocks, rows)
            assert sum(r[1] for r in rows) == len(fh.naive_walk(stream, fh.header_end(stream)[0])[0])
    # the planted BAMs of the call_bam tests, as call_bam reads them (one window)
    import index_helpers as ih
    for k, write in enumerate((call_helpers.write_planted_bam, ih.write_planted_small_blocks)):
        path = str(tmp_path / ("planted%d.bam" % k))
        write(path)
        stream, lens = fh.stream_of(path)
        rows = twin(fh.windows_of(stream, lens, 4096), len(call_helpers.CONTIGS))
        assert sum(r[6] for r in rows) == 0 and sum(r[1] for r in rows) > 40, rows
        for (w, _, c), r in zip(fh.windows_of(stream, lens, 4096), rows):
            assert r[7] == fh.rows_hash(w, fh.naive_walk(w, c)[0])
    for bb in (bam_writer.MAX_BLOCK, 4096):
        info, planted = fh.decoy_file(str(tmp_path / "decoy.bam"), block_bytes=bb)
        stream, lens = fh.stream_of(str(tmp_path / "decoy.bam"))
        rows = twin(fh.windows_of(stream, lens, 4096), 2)
        assert len(rows) == 1 and rows[0][6] == planted and rows[0][5] >= 1 and rows[0][1] == 40, rows


# ------------------------------------------------------------------------------------------------ CPU 2: the Python surface
def test_the_python_surface(tmp_path):
    assert call.DEFAULT_FRAME == "host"
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert all(s in names for s in NEW_SYMBOLS)
    L = _lib.lib()
    assert all(hasattr(L, s) for s in NEW_SYMBOLS)
    assert len(_abi.BAM_STRUCT_SIZES) == 3
    path = str(tmp_path / "a.bam")
    bam_writer.write_bam(path, fh.REFS, fh.short_records(20))
    with pytest.raises(ValueError, match="device inflate"):
        bam.BamFile(path, frame="device")
    with pytest.raises(ValueError, match="device inflate"):
        bam.BamFile(path, inflate="host", frame="device")
    for bad in ("gpu", 1, object()):
        with pytest.raises(ValueError, match="frame must be"):
            bam.BamFile(path, frame=bad)
    with bam.BamFile(path, frame="host") as bf:
        assert bf.frame is None and bf.set_frame(None) == "host"
        with pytest.raises(ValueError):
            bf.set_frame("device")
        ch = bf.records("7")
        assert not getattr(ch, "framed", False) and bf.frame_stats()["frame"] == "host"
        # csv_bam_chunk_lengths answers on the host route too
        l_name, l_seq = np.zeros(ch.n, np.int32), np.zeros(ch.n, np.int32)
        assert L.csv_bam_chunk_lengths(bf._h, l_name.ctypes.data, l_seq.ctypes.data) == 0
        assert (l_name - 1).tolist() == ch.name_columns()[1].tolist() and l_seq.tolist() == ch.sequence_columns()[1].tolist()
        assert L.csv_bam_chunk_fetch(bf._h, None, None) == _abi.E_STATE
    ref = {c: "A" * 10 for c, _ in fh.REFS}
    with pytest.raises(ValueError, match="inflate='host'"):
        call.call_bam(path, ref, Params.ont(), frame="device", inflate="host")
    with pytest.raises(ValueError, match="frame must be"):
        call.call_bam(path, ref, Params.ont(), frame="gpu")
    own, rest = cli.split_own(["a.bam", "--frame", "device", "-s", "3"])
    assert own.frame == "device" and rest == ["a.bam", "-s", "3"]
    assert cli.split_own(["a.bam"])[0].frame is None


# ------------------------------------------------------------------------------------------------ GPU 1: chunk parity
KEYS = ("slim", "rec_off", "rec_len", "host", "host_off")


def _image(ch):
    return tuple(np.asarray(getattr(ch, k)).tobytes() for k in KEYS) + (ch.n, ch.more, ch.stats["record_bytes"])


def _reads(bf, chroms, grid=None, ranges=None):
    """every kind of read the tests compare: -> list of images"""
    out = []
    for c in chroms:
        out.append(_image(bf.records(c)))
        for k in (1, 7, 65536):
            out.append([_image(ch) for ch in bf.chunks(c, chunk_records=k)])
        out.append(bf.count(c))
        for lo, hi in grid or ():
            out.append(_image(bf.records(c, lo, hi)))
        if ranges is not None:
            out.append(_image(bf.records(c, ranges=ranges)))
            out.append([_image(ch) for ch in bf.chunks(c, chunk_records=7, ranges=ranges)])
    return out


def _framed(ctx, path, wb=0, **kw):
    bf = bam.BamFile(path, threads=2, inflate=ctx, frame="device", **kw)
    if wb:
        bf.set_inflate(ctx, window_blocks=wb)
        bf.set_frame("device")
    return bf


GRID = [(0, 1), (1000, 1200), (1500, 1501), (2000, 4000), (3999, 10 ** 9), (0, 10 ** 9), (10 ** 8, 10 ** 9)]


@pytest.mark.gpu
def test_gpu_device_chunks_equal_the_host_chunks(ctx, plain):
    for path, wb in plain:
        chroms = ["7", "X", None] if path.endswith("two.bam") else ["7"]
        with bam.BamFile(path, threads=2, index=False) as bf:
            want = _reads(bf, chroms, GRID)
        with _framed(ctx, path, wb, index=False) as bf:
            ch = bf.records("7")                                               # (the reader's first read: every window is framed now, none is known yet)
            assert ch.framed and ch.stats["frame"] == "device" and ch.stats["frame_fallback_blocks"] == 0, (path, ch.stats)
            assert ch.stats["right_blocks"] >= 1 or ch.n == 0, (path, ch.stats)
            got = _reads(bf, chroms, GRID)
        assert got == want, path


@pytest.mark.gpu
def test_gpu_ranges_with_the_index_and_the_long_cigar(ctx, tmp_path):
    import bai_writer
    import test_bam_reader as tbr
    recs = fh.short_records(2000, step=60)
    path = str(tmp_path / "ix.bam")
    bam_writer.write_bam(path, fh.REFS, recs, block_bytes=3000)
    bai_writer.write_bai(path)
    ranges = [(1000, 1400), (20000, 20100), (40000, 41000), (70000, 70001)]
    with bam.BamFile(path, threads=2) as bf:
        assert bf.has_index
        want = _reads(bf, ["7"], GRID[:3], ranges)
    with _framed(ctx, path, 2) as bf:
        assert bf.has_index
        assert _reads(bf, ["7"], GRID[:3], ranges) == want
    # the 70 000-operation CG record, cut inside its array: one record exceeds a window of one block
    edge = str(tmp_path / "edge.bam")
    _, info = tbr.write_edge(edge)
    r6 = info["records"][6]
    tbr.write_edge(edge, cuts=[r6["aux"] + 11, r6["aux"] + 100001, r6["end"] - 1, r6["offset"] + 3])
    with bam.BamFile(edge, threads=2) as bf:
        want = _reads(bf, ["7"])
    for wb in (1, 2, 0):
        with _framed(ctx, edge, wb) as bf:
            assert _reads(bf, ["7"]) == want, wb


@pytest.mark.gpu
def test_gpu_only_rows_and_tables_cross_the_link(ctx, twin, tmp_path):
    """a read without a fetch: what the framing route copies down is the status bytes of the inflate, one verdict per framing run and
    one row per framed record; what it copies up is the compressed bytes, the tables of the inflate and of the framing, one pack row
    per selected record and the blocks the host had to inflate (none here) - no window and no image"""
    path = str(tmp_path / "a.bam")
    bam_writer.write_bam(path, fh.REFS, fh.short_records(500), block_bytes=3000)
    stream, lens = fh.stream_of(path)
    (win,) = fh.windows_of(stream, lens, 4096)
    (row,) = twin([win], 2)
    with _framed(ctx, path, index=False) as bf:
        ch = bf.records("7", 5000, 9000)                                       # a region: fewer records selected than framed
        st = ch.stats
        n_blocks = st["device_blocks"] + st["fallback_blocks"]
        assert 0 < ch.n < 500 and row[1] == 500 and n_blocks == len(lens) and st["fallback_blocks"] == 0
        assert st["frame_bytes_down"] == n_blocks + 32 * 1 + 40 * row[1], (st, row)
        tables = 28 * n_blocks + ((20 * n_blocks + 15) & ~15)
        assert st["frame_bytes_up"] == st["compressed_bytes"] + tables + 40 * ch.n, (st, ch.n)
        assert st["frame_bytes_down"] + st["frame_bytes_up"] < st["inflated_bytes"] and not ch.fetched
        cols = bam.decode(ctx, ch, host_outputs=False)
        assert cols["bytes_uploaded"] == 12 * ch.n and not ch.fetched
        n = bf.count("7")                                                      # the counting pass packs nothing
        st = bf.last_stats
        assert n == 500 and st["frame_bytes_up"] == 0 and st["frame_bytes_down"] == 0      # (the window is known: its rows are reused)
        # a second framing reader on the same context is refused, and frames on the host
        with bam.BamFile(path, inflate=ctx, index=False) as other:
            with pytest.raises(bam.BamError, match="one framing reader per context"):
                other.set_frame("device")
            assert other.frame is None and not getattr(other.records("7"), "framed", False)
        # an empty list of ranges: the same keys in the stats
        assert bf.records("7", ranges=[]).n == 0 and bf.last_stats["frame"] == "device"
    with _framed(ctx, path, index=False) as bf:                               # (the first reader left when it was closed)
        assert bf.records("7").n == 500


# ------------------------------------------------------------------------------------------------ GPU 2: decoys
@pytest.mark.gpu
def test_gpu_decoys_fall_back_and_change_nothing(ctx, twin, tmp_path):
    path = str(tmp_path / "decoy.bam")
    info, planted = fh.decoy_file(path)
    stream, lens = fh.stream_of(path)
    (row,) = twin(fh.windows_of(stream, lens, 4096), 2)
    with bam.BamFile(path, threads=2) as bf:
        want = _image(bf.records("7"))
    with _framed(ctx, path) as bf:
        ch = bf.records("7")
        st = ch.stats
        assert _image(ch) == want and ch.n == 40
    assert st["frame_fallback_blocks"] == planted == row[6] and st["right_blocks"] == row[5], (st, row)


# ------------------------------------------------------------------------------------------------ GPU 3: damaged files
def _both_raise(ctx, path, chrom="7"):
    texts = []
    for framed in (False, True):
        with (_framed(ctx, path) if framed else bam.BamFile(path, threads=2)) as bf:
            with pytest.raises(bam.BamError) as ei:
                for ch in bf.chunks(chrom, chunk_records=50):
                    ch.slim
            texts.append(str(ei.value))
            st = bf.inflate_stats()
    assert texts[0] == texts[1], texts
    return texts[0], st


@pytest.mark.gpu
def test_gpu_damaged_files_raise_the_same_text(ctx, tmp_path):
    recs = fh.short_records(400)
    p = lambda n: str(tmp_path / n)                                                # noqa: E731
    info = bam_writer.write_bam(p("full.bam"), fh.REFS, recs, cuts="record")
    blob = open(p("full.bam"), "rb").read()
    # block_size < 32 on the true chain
    open(p("small.bam"), "wb").write(blob[:-28] + bam_writer.bgzf_block(struct.pack("<i", 31) + b"\0" * 40) + bam_writer.EOF_BLOCK)
    assert "block_size < 32" in _both_raise(ctx, p("small.bam"))[0]
    # a file that ends inside a record, and inside a block_size word
    open(p("short.bam"), "wb").write(blob[:-28] + bam_writer.bgzf_block(b"\x40\x00\x00\x00" + b"\0" * 20) + bam_writer.EOF_BLOCK)
    assert "ends inside a record" in _both_raise(ctx, p("short.bam"))[0]
    open(p("short2.bam"), "wb").write(blob[:-28] + bam_writer.bgzf_block(b"\x40\x00") + bam_writer.EOF_BLOCK)
    assert "ends inside a record" in _both_raise(ctx, p("short2.bam"))[0]
    # fields that exceed block_size: l_seq of record 200 says more than the record holds
    stream, lens = fh.stream_of(p("full.bam"))
    bad = bytearray(stream)
    struct.pack_into("<I", bad, info["records"][200]["fixed"] + 16, 1 << 20)
    out, o = [], 0
    for ln in lens[:-1]:
        out.append(bam_writer.bgzf_block(bytes(bad[o : o + ln]))); o += ln
    open(p("fields.bam"), "wb").write(b"".join(out) + bam_writer.EOF_BLOCK)
    assert "exceed its block_size" in _both_raise(ctx, p("fields.bam"))[0]
    # a flipped payload byte: one block inflated on the host, whose verdict stands
    blocks, o = [], 0
    while o < len(blob):
        size = struct.unpack_from("<H", blob, o + 16)[0] + 1
        blocks.append((o, size)); o += size
    off, size = blocks[300]
    flipped = bytearray(blob)
    flipped[off + 18 + (size - 26) // 2] ^= 0x10
    open(p("crc.bam"), "wb").write(bytes(flipped))
    text, st = _both_raise(ctx, p("crc.bam"))
    assert "byte %d does not inflate" % off in text and st["fallback_blocks"] == 1


# ------------------------------------------------------------------------------------------------ GPU 4: the consumers
@pytest.mark.gpu
def test_gpu_framed_consumers_equal_their_host_twins(ctx, tmp_path):
    from cutesv_amd.engine import CsvError
    path = str(tmp_path / "planted.bam")
    call_helpers.write_planted_bam(path)
    out = {}
    for route in ("host", "device"):
        with (_framed(ctx, path) if route == "device" else bam.BamFile(path, threads=2)) as bf:
            rebuild.name_pool_reset(ctx)
            ch = bf.records("chrA")
            cols = bam.decode(ctx, ch, host_outputs=True)
            first = rebuild.name_pool_append_chunk(ctx, ch)
            names = rebuild.name_pool_get(ctx, np.arange(first, first + ch.n))
            want = (np.arange(ch.n) % 3 != 0).astype(np.uint8)
            if route == "device":
                extract.upload_read_sequences(ctx, ch, want=want)
                assert not ch.fetched                                          # no image came down for any of the three
            else:
                extract.upload_read_sequences(ctx, ch.host, *ch.sequence_columns(), want=want)
            info = extract.seq_info(ctx)
            out[route] = (ch.n, {k: v.tobytes() for k, v in cols.items() if isinstance(v, np.ndarray)}, cols["n_ops"], cols["n_sa"], names, info["reads_uploaded"],
                          [ch.name(i) for i in range(0, ch.n, 17)], [ch.sequence(i) for i in range(0, ch.n, 29)])
            if route == "device":
                assert cols["bytes_uploaded"] == 12 * ch.n and ch.fetched
                bf.records("chrB")                                             # the next read: the device chunk of `ch` is gone
                with pytest.raises(bam.BamError, match="device chunk is gone"):
                    bam.decode(ctx, bf_chunk_unfetched(ch))
                bf.count("chrA")                                               # a counting pass leaves no chunk at all
                L = _lib.lib()
                o = _abi.BamOut()
                import ctypes as C
                assert L.csv_bam_decode_framed(ctx._h, C.byref(o)) == _abi.E_STATE
                assert L.csv_name_pool_append_framed(ctx._h, None) == _abi.E_STATE
                assert L.csv_seq_reads_framed(ctx._h, None) == _abi.E_STATE
    assert out["host"] == out["device"] and out["host"][0] > 20
    rebuild.name_pool_reset(ctx)


def bf_chunk_unfetched(ch):
    """the same device chunk as somebody who never fetched it sees it"""
    ch._images = None
    return ch


def _seq_row(ctx, k):
    """the bases of pool row k, None for a row without a sequence"""
    from cutesv_amd.engine import CsvError
    try:
        return rebuild.seq_pool_get(ctx, np.array([k]))
    except CsvError:
        return None


@pytest.mark.gpu
def test_gpu_task_to_pool_fills_the_same_pools(ctx, tmp_path):
    path = str(tmp_path / "planted.bam")
    call_helpers.write_planted_bam(path)
    cp = call.CallParams(Params.ont(min_support=3))
    names = sorted(c for c, _ in call_helpers.CONTIGS)
    crank = {c: i for i, c in enumerate(names)}
    out = {}
    for route in ("host", "device"):
        with (_framed(ctx, path) if route == "device" else bam.BamFile(path, threads=2)) as bf:
            rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
            seg_of = {t: ti * len(names) for ti, t in enumerate(call.TYPES)}
            seg_base = [seg_of[t] for t in ("DEL", "INS", "DUP", "INV", "TRA")]
            res = []
            for c in names:
                r = extract.task_to_pool(ctx, bf, c, 0, 1 << 40, crank, *cp.pipe_args(), seg_of["INS"] + crank[c], seg_of["DEL"] + crank[c], seg_base, None,
                                         name_pool=True, seq_pool=True)
                res.append({k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items()})
            n = rebuild.pool_rows(ctx)
            out[route] = (res, n, rebuild.seq_pool_rows(ctx), rebuild.name_pool_get(ctx, np.arange(rebuild.name_pool_rows(ctx))),
                          [_seq_row(ctx, k) for k in range(n)])
    assert out["host"] == out["device"] and out["host"][1] > 20
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_a_framed_read_leaves_the_decode_columns_and_a_kept_rebuild_alone(ctx, tmp_path):
    import test_bam_reader as tbr
    import test_call_bam as tcb
    path = str(tmp_path / "edge.bam")
    tbr.write_edge(path)
    other = str(tmp_path / "other.bam")
    bam_writer.write_bam(other, fh.REFS, fh.short_records(300), block_bytes=4096)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    use = np.ones(ch.n, np.uint8)
    keys = ("ins_read", "ins_pos", "ins_len", "ins_piece0", "ins_npiece", "piece_qoff", "piece_len", "del_read", "del_pos", "del_len")
    with _framed(ctx, other, 2) as fb:
        cols = bam.decode(ctx, ch)
        want = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
        cols = bam.decode(ctx, ch)
        assert fb.records("7").n == 300                                        # windows, framing kernels, the pack kernel
        got = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
        assert want["n_sig_ins"] > 100
        for k in keys:
            assert np.array_equal(got[k], want[k]), k
        seqs, rb = tcb.alt_pool(ctx)
        src = rb["src_row"]
        ins_rows = np.flatnonzero(src < len(tcb.ALT_LENS))
        clip = np.asarray([len(seqs[int(src[r])]) for r in ins_rows], np.int64)
        want = rebuild.alt_gather_host(seqs, src, ins_rows, clip)
        assert fb.records("7", 2000, 3000).n > 0
        got = rebuild.alt_gather(ctx, ins_rows, clip)
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and len(want[0]) > 1000
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU 5: call_bam, the command lines
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_call")
    import index_helpers as ih
    path = str(d / "planted.bam")
    ref = ih.write_planted_small_blocks(path)                                  # (with its index: under include_bed a task reads its regions only)
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    bed = str(d / "regions.bed")
    with open(bed, "w") as f:
        for c, n in call_helpers.CONTIGS:
            f.write("%s\t%d\t%d\n" % (c, 0, n // 2))
    return path, ref, fa, bed


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("plain", "genotype", "bed"))
def test_gpu_call_bam_gives_the_same_text_on_both_routes(ctx, planted, case, tmp_path):
    path, ref, fa, bed = planted
    genotype = case == "genotype"
    cp = call.CallParams(Params.ont(min_support=3, genotype=genotype))
    kw = dict(tra_gt="alignments" if case == "genotype" else None, report_readid=True, include_bed=bed if case == "bed" else None)
    th, td = {}, {}
    host, svid_h = call.call_bam(path, ref, cp, ctx=ctx, frame="host", timings=th, sigs_dir=str(tmp_path), **kw)
    sigs_h = {t: open(str(tmp_path / (t + ".sigs")), "rb").read() for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    dev, svid_d = call.call_bam(path, ref, cp, ctx=ctx, frame="device", timings=td, sigs_dir=str(tmp_path), **kw)
    sigs_d = {t: open(str(tmp_path / (t + ".sigs")), "rb").read() for t in ("DEL", "INS", "DUP", "INV", "TRA")}
    assert host.count("\n") >= 3 and "SVTYPE=INS" in host
    assert dev == host and svid_d.tolist() == svid_h.tolist() and sigs_d == sigs_h and len(sigs_h["INS"]) > 500
    assert "ms_frame" in th and "ms_frame" in td and td["ms_inflate"] > 0
    # a reader that was handed in frames on the call's context during the call and has its own settings back afterwards
    with bam.BamFile(path) as bf:
        seen, read = [], bf._read
        bf._read = lambda *a, **k: (read(*a, **k), seen.append(dict(bf.last_stats)))[0]
        assert call.call_bam(bf, ref, cp, ctx=ctx, frame="device", **kw)[0] == host
        assert bf.inflate is None and bf.frame is None and len(seen) >= 2
        assert all(s["inflate"] == "device" and s["frame"] == "device" and s["frame_fallback_blocks"] == 0 for s in seen)
        assert call.call_bam(bf, ref, cp, ctx=ctx, **kw)[0] == host
        assert "frame" not in bf.last_stats


@pytest.mark.gpu
def test_gpu_command_lines_take_frame(planted, tmp_path, capsys):
    path, ref, fa, bed = planted
    wd = str(tmp_path / "work")
    os.mkdir(wd)
    outs = {}
    for route in ("host", "device"):
        out = str(tmp_path / (route + ".vcf"))
        assert cli.main([path, fa, out, wd, "-s", "3", "--genotype", "--frame", route]) == 0
        lines = open(out, "rb").read().split(b"\n")
        outs[route] = [ln for ln in lines if not ln.startswith(b"##fileDate=") and not ln.startswith(b"##CommandLine=")]
        body = str(tmp_path / (route + ".body.vcf"))
        assert call.main([path, fa, "-o", body, "--preset", "ont", "--min_support", "3", "--frame", route]) == 0
        outs[route + " body"] = open(body, "rb").read()
    assert outs["host"] == outs["device"] and len(outs["host"]) > 20
    assert outs["host body"] == outs["device body"] and outs["host body"].count(b"\n") >= 5
    capsys.readouterr()
    assert bam.main([path, "--inflate", "device", "--frame", "device"]) == 0
    dev = capsys.readouterr().out
    assert bam.main([path]) == 0
    assert capsys.readouterr().out == dev and "chrA\t" in dev
