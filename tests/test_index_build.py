"""Building the BAM index a file came without: BamFile.build_index on every reader route against the twin -
tests/bai_writer.py's bytes with its defaults (filled linear index, pseudo-bins, n_no_coor) - over the grid BAM, the planted BAM, block
sizes that put records on block boundaries, and crafted edges; the refusals and their texts; the reader after a build; the C entries;
the writing; the command lines; and, under the sanitizers, the core alone (tests/index_core_main.cpp).  On the GPU the device route
(device inflate + device framing, the index kernels over rows that stay on the device) must give the same bytes at every window
size, copy down no row, and leave the rest of the context alone."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_writer
import frame_helpers as fh
import index_build_helpers as H
import index_helpers as ih
from cutesv_amd import _abi, _lib, bam, call, cli
from cutesv_amd.columns import Params, TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("grid", "planted", "grid_bb64", "grid_bb200", "grid_bb65280", "grid_cg", "grid_level0", "many", "header_only", "tail_only", "one_record", "pos0", "window_edges",
         "placed_unmapped", "levels", "bin_again")
WINDOWS = (1, 2, 64, 0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{name: (path, the twin's info)} of every file of the byte comparison, written once"""
    d = tmp_path_factory.mktemp("index_build")
    out = {name: (path, H.twin(path)) for name, path in H.parity_files(d)}
    assert tuple(out) == FILES
    return out


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _no_index_files(path):
    d = os.path.dirname(path)
    return [f for f in os.listdir(d) if f.startswith(os.path.basename(path)) and f != os.path.basename(path)] == []


# ------------------------------------------------------------------------------------------------ CPU 1, 2: the bytes
def test_the_files_are_what_the_tests_need(files):
    """the grid is the issue's file; the crafted edges hold what their names say"""
    _, info = files["grid"]
    assert len(info["records"]) == 410 and H.twin_runs(info) == 26 and len(info["bytes"]) == 1416
    for name in ("grid_bb64", "grid_bb200", "grid_bb65280"):                   # records that start on a block boundary, and one that ends on the last one
        _, info = files[name]
        assert sum(1 for r in info["records"] if r["voff"] & 0xffff == 0) >= 8 and info["records"][-1]["voff_end"] == info["blocks"][-1][0] << 16
    _, info = files["many"]
    assert len(info["records"]) == 2500 > 2 * 1024 and len(info["blocks"]) < 64      # several tiles of the scan, one window at every size but 1 and 2
    _, info = files["levels"]
    bins = sorted(info["refs"][0]["bins"])
    level = lambda b: sum(b >= base for base in (1, 9, 73, 585, 4681))           # noqa: E731
    assert sorted(level(b) for b in bins) == [0, 1, 2, 3, 4, 5] and len(info["refs"][0]["ioffset"]) == 1 << 15
    _, info = files["bin_again"]
    assert sorted(len(c) for c in info["refs"][0]["bins"].values()) == [1, 2]
    _, info = files["window_edges"]
    assert [len(R["ioffset"]) for R in info["refs"]] == [6, 0, 0]
    _, info = files["placed_unmapped"]
    assert (info["refs"][0]["n_mapped"], info["refs"][0]["n_unmapped"], info["n_no_coor"]) == (2, 2, 2)


@pytest.mark.parametrize("name", FILES)
def test_host_bytes_equal_the_twins(files, name):
    path, info = files[name]
    with bam.BamFile(path, index=False) as bf:
        assert not bf.has_index
        st = bf.build_index()
        got = bf.index_bytes()
        assert got == info["bytes"], (name, len(got), len(info["bytes"]))
        assert st["records"] == len(info["records"]) and st["runs"] == H.twin_runs(info) and st["index_bytes"] == len(got)
        assert st["inflate"] == "host" and st["frame"] == "host" and st["bytes_down"] == 0 and st["written"] is None
        assert bf.has_index and H.same_stats(bf, info, bf.references)
    assert _no_index_files(path)


# ------------------------------------------------------------------------------------------------ CPU 3: refusals
def _refused(bf, path, ordinal, text, **kw):
    with pytest.raises(bam.BamError) as ei:
        bf.build_index(**kw)
    msg = str(ei.value)
    assert msg.startswith(path + ": cannot build the index: record %d " % ordinal) and text in msg, msg
    assert not bf.has_index
    with pytest.raises(bam.BamError, match="no built index"):
        bf.index_bytes()
    with pytest.raises(bam.BamError, match="no index is loaded"):
        bf.index_statistics()
    return msg


@pytest.mark.parametrize("name", sorted(H.REFUSALS))
def test_refusals_name_the_file_and_the_record(tmp_path, name):
    path, ordinal, text = H.refusal_file(tmp_path, name, block_bytes=300)
    with bam.BamFile(path, index=False) as bf:
        _refused(bf, path, ordinal, text, write=True)
        assert os.listdir(tmp_path) == [os.path.basename(path)]              # no index, no temporary file
        assert sum(bf.count(c) for c in bf.references) >= 1                   # the reader still reads
    with pytest.raises(bam.BamError, match="cannot build the index"):
        bam.BamFile(path, index="build")


def test_a_refused_build_keeps_the_index_the_reader_had(tmp_path, files):
    path, ordinal, text = H.refusal_file(tmp_path, "pos_order")
    good, info = files["grid"]
    with bam.BamFile(good, index=False) as bf:
        bf.build_index()
        want = bf.index_bytes()
    with bam.BamFile(path, index=False) as bf:
        with pytest.raises(bam.BamError, match="record %d is out of coordinate order" % ordinal):
            bf.build_index()
        assert not bf.has_index
    assert want == info["bytes"]


# ------------------------------------------------------------------------------------------------ CPU 4: the reader after a build
def test_the_reader_after_a_build(files, tmp_path):
    path, info = files["grid"]
    bai = str(tmp_path / "twin.bai")
    with open(bai, "wb") as f:
        f.write(info["bytes"])
    with bam.BamFile(path, index=False) as built, bam.BamFile(path, index=False) as plain, bam.BamFile(path, index=bai) as loaded:
        built.build_index()
        assert built.has_index and not plain.has_index
        assert H.same_stats(built, info, built.references)
        assert built.index_statistics() == [("one", 203, 1, 204), ("none", 0, 0, 0), ("two", 201, 0, 201)] and built.no_coordinate == 5
        seeks = 0
        for chrom, (_, length), R in zip(built.references, ih.REFS, info["refs"]):
            pts = ih.grid_points(len(R["ioffset"]), length)
            for beg, end in [(pts[i], pts[min(i + 3, len(pts) - 1)]) for i in range(0, len(pts), 5)] + [(0, length), (12 * ih.WINDOW - 90, 12 * ih.WINDOW), (44 * ih.WINDOW, bam.ALL)]:
                a, b, c = built.records(chrom, beg, end), plain.records(chrom, beg, end), loaded.records(chrom, beg, end)
                assert ih.same_chunk(a, b), (chrom, beg, end)
                assert ih.same_chunk(a, c) and built.index_block(chrom, beg) == loaded.index_block(chrom, beg), (chrom, beg, end)
                seeks += built.index_block(chrom, beg) > 0
        assert seeks > 5                                                      # the built index moves starting points exactly as the loaded one does
        assert built.index_block("one", 44 * ih.WINDOW) > built.index_block("one", 0) >= 0
        assert ih.same_chunk(built.records(None), plain.records(None)) and built.records(None).n == 5


def test_index_build_on_open(files, tmp_path):
    path, info = files["planted"]
    with bam.BamFile(path, index="build") as bf:                              # none beside the file: built in memory, nothing written
        assert bf.has_index and bf.index_stats["records"] == len(info["records"]) and bf.index_bytes() == info["bytes"]
    assert _no_index_files(path)
    beside = str(tmp_path / "p.bam")
    shutil.copy(path, beside)
    with open(beside + ".bai", "wb") as f:
        f.write(info["bytes"])
    with bam.BamFile(beside, index="build") as bf:                            # one beside the file: loaded, not built
        assert bf.has_index and bf.index_stats is None
        with pytest.raises(bam.BamError, match="no built index"):
            bf.index_bytes()


# ------------------------------------------------------------------------------------------------ CPU 5: the C entries
def test_csv_bam_index_bytes(files, tmp_path):
    path, info = files["grid"]
    L = _lib.lib()
    out = str(tmp_path / "g.bai")
    with bam.BamFile(path, index=False) as bf:
        need = C.c_int64(-1)
        assert L.csv_bam_index_bytes(bf._h, None, 0, C.byref(need)) == _abi.E_STATE and need.value == 0      # no index at all
        bf.build_index(write=out)
        data = open(out, "rb").read()
        n = len(data)
        buf = np.full(n + 8, 0xA5, np.uint8)
        assert L.csv_bam_index_bytes(bf._h, buf.ctypes.data, n - 1, C.byref(need)) == _abi.E_CAPACITY and need.value == n
        assert (buf == 0xA5).all()                                            # nothing stored
        assert L.csv_bam_index_bytes(bf._h, buf.ctypes.data, n, C.byref(need)) == _abi.OK and need.value == n
        assert buf[:n].tobytes() == data == info["bytes"] and (buf[n:] == 0xA5).all()
        rec, runs, ms, up, dn, fr, iw = C.c_int64(), C.c_int64(), C.c_double(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        assert L.csv_bam_index_build_stats(bf._h, C.byref(rec), C.byref(runs), C.byref(ms), C.byref(up), C.byref(dn), C.byref(fr), C.byref(iw)) == _abi.OK
        assert (rec.value, runs.value, up.value, dn.value, fr.value, iw.value) == (410, 26, 0, 0, 0, 0)
        assert L.csv_bam_index_build(bf._h, 1, None) == _abi.E_INVALID        # no flag is defined
        bf.load_index(out)                                                    # a loaded index keeps no bins
        assert bf.has_index and L.csv_bam_index_bytes(bf._h, buf.ctypes.data, n, C.byref(need)) == _abi.E_STATE
        bf.build_index()
        assert bf.index_bytes() == data
        bf.drop_index()
        assert L.csv_bam_index_bytes(bf._h, buf.ctypes.data, n, C.byref(need)) == _abi.E_STATE


# ------------------------------------------------------------------------------------------------ CPU 6: writing
def test_writing_the_index(files, tmp_path):
    path, info = files["grid"]
    mine = str(tmp_path / "grid.bam")
    shutil.copy(path, mine)
    with bam.BamFile(mine, index=False) as bf:
        st = bf.build_index(write=True)
        assert st["written"] == mine + ".bai" and open(mine + ".bai", "rb").read() == info["bytes"]
        assert sorted(os.listdir(tmp_path)) == ["grid.bam", "grid.bam.bai"]   # the temporary file is gone
        with pytest.raises(FileExistsError):
            bf.build_index(write=True)
        with open(mine + ".bai", "wb") as f:
            f.write(b"old")
        with pytest.raises(FileExistsError):
            bf.build_index(write=mine + ".bai")
        assert open(mine + ".bai", "rb").read() == b"old"
        bf.build_index(write=True, overwrite=True)
        assert open(mine + ".bai", "rb").read() == info["bytes"]
        other = str(tmp_path / "elsewhere.bai")
        assert bf.build_index(write=other)["written"] == other and open(other, "rb").read() == info["bytes"]
    with bam.BamFile(mine) as fresh, bam.BamFile(mine, index=other) as there:  # a fresh reader loads what was written
        assert fresh.has_index and there.has_index and H.same_stats(fresh, info, fresh.references) and H.same_stats(there, info, there.references)
        assert fresh.index_block("two", 40 * ih.WINDOW) == there.index_block("two", 40 * ih.WINDOW) > 0
    bad, _, _ = H.refusal_file(tmp_path, "ref_order")
    before = sorted(os.listdir(tmp_path))
    with bam.BamFile(bad, index=False) as bf:
        with pytest.raises(bam.BamError):
            bf.build_index(write=True)
    assert sorted(os.listdir(tmp_path)) == before                             # a failed build leaves no file and no temporary file


# ------------------------------------------------------------------------------------------------ CPU 7: the ABI
def test_the_header_declares_what_is_bound_and_exported():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+CSV_ABI_VERSION\s+9\b", header) and _abi.ABI_VERSION == 9 and _lib.lib().csv_abi_version() == 9
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    for name, n_args in (("csv_bam_index_build", 3), ("csv_bam_index_bytes", 4), ("csv_bam_index_build_stats", 8)):
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(bound[name][1]) and bound[name][0] is C.c_int, name
        assert getattr(_lib.lib(), name) is not None
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert {"csv_bam_index_build", "csv_bam_index_bytes", "csv_bam_index_build_stats"} <= names
    assert not {n for n in names if n.startswith("csv_index_")}               # the reader's way to the device stays inside the library
    assert {n for n in names if n.startswith("csv_")} == set(bound)           # everything exported is declared and bound, and the other way round


# ------------------------------------------------------------------------------------------------ CPU 8: the core under the sanitizers
def test_the_core_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/index_core_main.cpp")
    exe = str(tmp_path / "index_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "index_core_main.cpp")], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok ") and int(p.stdout.split()[1]) > 5000, (p.stdout[-2000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ CPU 9: the command lines
def test_the_command_lines(files, tmp_path, capsys):
    path, info = files["grid"]
    mine = str(tmp_path / "g.bam")
    shutil.copy(path, mine)
    assert bam.main([mine, "--index"]) == 0
    assert open(mine + ".bai", "rb").read() == info["bytes"] and "wrote %s.bai: 1416 bytes, 410 records" % mine in capsys.readouterr().out
    with pytest.raises(SystemExit):                                           # it exists: --force replaces it
        bam.main([mine, "--index"])
    assert "--force" in capsys.readouterr().err
    with open(mine + ".bai", "wb") as f:
        f.write(b"old")
    assert bam.main([mine, "--index", "--force"]) == 0 and open(mine + ".bai", "rb").read() == info["bytes"]
    out = str(tmp_path / "there.bai")
    assert bam.main([mine, "--index", "--index_out", out]) == 0 and open(out, "rb").read() == info["bytes"]
    with pytest.raises(SystemExit):
        bam.main([mine, "--index_out", out])
    p = subprocess.run([sys.executable, "-m", "cutesv_amd.bam", mine, "--idxstats"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.splitlines()[0] == "one\t2000000\t203\t1", p.stderr[-2000:]
    own, rest = cli.split_own(["a.bam", "--build_index", "ref.fa", "-s", "3"])
    assert own.build_index is True and rest == ["a.bam", "ref.fa", "-s", "3"]
    assert cli.split_own(["a.bam"])[0].build_index is False
    assert cli.parse_args(["a", "b", "c", "d", "-b", "5"]).batches == 5         # (an abbreviation of cuteSV's own flags is not shadowed)


# ================================================================================================ GPU
def _framed(ctx, path, wb=0, **kw):
    bf = bam.BamFile(path, threads=2, inflate=ctx, frame="device", **kw)
    if wb:
        bf.set_inflate(ctx, window_blocks=wb)
        bf.set_frame("device")
    return bf


def _first_ordinals(path, wb):
    """the ordinal of every window's first record, for the windows the reader forms at `wb` blocks"""
    stream, lens = fh.stream_of(path)
    out, n = [], 0
    for w, _, c in fh.windows_of(stream, lens, wb or 4096):
        out.append(n)
        n += len(fh.naive_walk(w, c)[0])
    return out


# ------------------------------------------------------------------------------------------------ GPU 1, 2: bytes and the byte counter
@pytest.mark.gpu
@pytest.mark.parametrize("name", FILES)
def test_gpu_device_bytes_equal_host_bytes_equal_the_twins(ctx, files, name):
    path, info = files[name]
    with bam.BamFile(path, index=False) as bf:
        bf.build_index()
        host = bf.index_bytes()
    with bam.BamFile(path, inflate=ctx, index=False) as bf:                   # device inflate + host framing: the host loop out of the page-locked window
        st = bf.build_index()
        assert bf.index_bytes() == host and st["inflate"] == "device" and st["frame"] == "host" and st["runs"] == H.twin_runs(info)
    assert host == info["bytes"]
    for wb in WINDOWS:
        with _framed(ctx, path, wb, index=False) as bf:
            st = bf.build_index()
            assert bf.index_bytes() == host, (name, wb)
            assert st["frame"] == "device" and st["records"] == len(info["records"]) and H.same_stats(bf, info, bf.references)
            # GPU 2: the rows stay on the device.  Run rows: the twin's chunks, and one more for every window seam inside a run
            assert st["runs"] == H.seam_rows(info, _first_ordinals(path, wb)), (name, wb, st)
            assert st["bytes_down"] == H.expected_bytes_down(info, st, bf.lengths), (name, wb, st)
            assert st["index_windows"] <= st["frame_runs"] and st["frame_fallback_blocks"] == 0 and st["fallback_blocks"] == 0
            if info["records"]:
                # one status byte per block from the first record's block on, each inflated once; the empty end-of-file block only when a window reaches it
                ustart = np.r_[0, np.cumsum([b[2] for b in info["blocks"]])]
                b_first = int(np.searchsorted(ustart, info["records"][0]["off"], side="right") - 1)
                assert st["device_blocks"] in (len(info["blocks"]) - b_first - 1, len(info["blocks"]) - b_first), (name, wb, st)


@pytest.mark.gpu
def test_gpu_small_windows_cut_where_it_can_go_wrong(ctx, files):
    """what the small windows of the comparison above really contain: a run that continues over a seam, a reference change and the
    unmapped tail on a window's first record, and a window that holds no complete record"""
    path, info = files["grid_bb200"]
    recs = info["records"]
    firsts = _first_ordinals(path, 1)
    key = lambda r: (r["refid"], bam_writer.reg2bin(max(r["pos"], 0), max(r["end"], 1)))       # noqa: E731
    assert sum(1 for o in firsts if o and key(recs[o]) == key(recs[o - 1]) and recs[o]["refid"] >= 0) > 20
    with _framed(ctx, files["grid_bb64"][0], 1, index=False) as bf:        # blocks of 64 bytes: most records straddle one
        st = bf.build_index()
        assert st["frame_runs"] > st["index_windows"] > 50                    # framing runs that found no complete record: the window grew
    # a reference change and the tail's first record at the head of a window: the files cut at those records
    for name in ("grid_bb64", "grid_bb65280"):
        path, info = files[name]
        recs = info["records"]
        on_cut = {o for o, r in enumerate(recs) if r["voff"] & 0xffff == 0}
        assert any(recs[o]["refid"] != recs[o - 1]["refid"] and recs[o]["refid"] >= 0 for o in on_cut if o) and any(recs[o]["refid"] < 0 <= recs[o - 1]["refid"] for o in on_cut if o)


# ------------------------------------------------------------------------------------------------ GPU 3: decoys
@pytest.mark.gpu
def test_gpu_the_decoy_file(ctx, tmp_path):
    path = str(tmp_path / "decoy.bam")
    _, planted = fh.decoy_file(path)
    info = H.twin(path)
    with bam.BamFile(path, index=False) as bf:
        bf.build_index()
        host = bf.index_bytes()
    with _framed(ctx, path, index=False) as bf:
        st = bf.build_index()
        assert bf.index_bytes() == host == info["bytes"] and st["records"] == 40
        assert st["frame_fallback_blocks"] == planted and st["right_blocks"] >= 1


# ------------------------------------------------------------------------------------------------ GPU 4: a damaged block
@pytest.mark.gpu
def test_gpu_a_flipped_payload_byte(ctx, tmp_path):
    path = str(tmp_path / "crc.bam")
    bam_writer.write_bam(path, fh.REFS, fh.short_records(400), cuts="record")
    blob = bytearray(open(path, "rb").read())
    blocks, o = [], 0
    while o < len(blob):
        size = struct.unpack_from("<H", blob, o + 16)[0] + 1
        blocks.append((o, size)); o += size
    off, size = blocks[300]
    blob[off + 18 + (size - 26) // 2] ^= 0x10
    open(path, "wb").write(bytes(blob))
    texts = []
    for framed in (False, True):
        with (_framed(ctx, path, index=False) if framed else bam.BamFile(path, index=False)) as bf:
            with pytest.raises(bam.BamError) as ei:
                bf.build_index(write=True)
            texts.append(str(ei.value))
            assert not bf.has_index
            with pytest.raises(bam.BamError, match="no built index"):
                bf.index_bytes()
    assert texts[0] == texts[1] and "byte %d does not inflate" % off in texts[0], texts
    assert os.listdir(tmp_path) == ["crc.bam"]


# ------------------------------------------------------------------------------------------------ GPU 5: refusals
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(H.REFUSALS))
def test_gpu_refusals_give_the_same_texts(ctx, tmp_path, name):
    path, ordinal, text = H.refusal_file(tmp_path, name, block_bytes=300)
    with bam.BamFile(path, index=False) as bf:
        want = _refused(bf, path, ordinal, text)
    for wb in (0, 1):
        with _framed(ctx, path, wb, index=False) as bf:
            assert _refused(bf, path, ordinal, text, write=True) == want
            assert sum(bf.count(c) for c in bf.references) >= 1
    assert os.listdir(tmp_path) == [os.path.basename(path)]


# ------------------------------------------------------------------------------------------------ GPU 6, 7: call_bam and the command line
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted BAM with small blocks twice: with the twin-written .bai beside it, and without"""
    d = tmp_path_factory.mktemp("index_build_call")
    with_bai, without = str(d / "with.bam"), str(d / "without.bam")
    ref = ih.write_planted_small_blocks(with_bai)
    shutil.copy(with_bai, without)
    bed = str(d / "two.bed")
    with open(bed, "w") as f:
        f.write("chrA\t9000\t11000\nchrA\t29500\t30500\n")
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return with_bai, without, ref, bed, fa, d


def _sigs(d):
    return {t: open(os.path.join(d, t + ".sigs"), "rb").read() for t in TYPES}


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("bed", [False, True])
def test_gpu_call_bam_builds_the_index_it_lacks(ctx, planted, tmp_path, route, bed):
    with_bai, without, ref, bed_path, _, d = planted
    cp = call.CallParams(Params.ont(min_support=3))
    kw = dict(ctx=ctx, task_cut="index", cut_threads=1, include_bed=bed_path if bed else None, frame=route, tra_gt="off" if bed else None)
    outs = []
    for path, index in ((with_bai, None), (without, "build")):
        sd = tmp_path / ("sigs_%s" % index)
        sd.mkdir()
        tm, rs = {}, {}
        text, svid = call.call_bam(path, ref, cp, index=index, sigs_dir=str(sd), timings=tm, read_stats=rs, **kw)
        outs.append((text, svid.tolist(), _sigs(str(sd)), rs["compressed_bytes"], rs["task_records"]))
        assert ("ms_index" in tm) == (index == "build")
    assert outs[0] == outs[1] and outs[0][0].count("\n") >= 1
    assert sorted(os.listdir(d)) == ["ref.fa", "two.bed", "with.bam", "with.bam.bai", "without.bam"]      # nothing was written
    with pytest.raises(ValueError, match="index"):
        call.call_bam(without, ref, cp, **kw)
    tm = {}
    call.call_bam(with_bai, ref, cp, index="build", timings=tm, **kw)       # an index beside the file: loaded, nothing built
    assert tm["ms_index"] < 50.0


@pytest.mark.gpu
def test_gpu_the_command_line_builds_the_index(planted, tmp_path, capsys):
    with_bai, without, ref, bed_path, fa, d = planted
    body = lambda p: "".join(ln for ln in open(p) if not ln.startswith("#"))       # noqa: E731
    work = tmp_path / "work"
    work.mkdir()
    args = [None, fa, None, str(work), "-s", "3", "-t", "1", "-include_bed", bed_path]
    outs = {}
    for name, path, extra in (("bai", with_bai, []), ("built", without, ["--build_index"]), ("built_device", without, ["--build_index", "--frame", "device"]),
                              ("uniform", without, []), ("bai_flag", with_bai, ["--build_index"])):
        args[0], args[2] = path, str(tmp_path / (name + ".vcf"))
        assert cli.main(args + extra) == 0
        outs[name] = (body(args[2]), capsys.readouterr().err)
    assert outs["bai"][0] == outs["built"][0] == outs["built_device"][0] == outs["bai_flag"][0] and outs["bai"][0].count("\n") >= 1
    assert "one is built in memory" in outs["built"][1] and "index" in outs["built"][1] and "uniform cut" not in outs["built"][1]
    assert "uniform cut" in outs["uniform"][1] and "built in memory" not in outs["uniform"][1] and "no BAM index" not in outs["bai_flag"][1]
    assert "without.bam.bai" not in os.listdir(d)
    dev = str(tmp_path / "dev.bai")
    assert bam.main([without, "--index", "--index_out", dev, "--inflate", "device", "--frame", "device"]) == 0
    assert open(dev, "rb").read() == open(with_bai + ".bai", "rb").read() and "frame device" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ GPU 8: isolation
@pytest.mark.gpu
def test_gpu_a_build_leaves_the_decode_columns_and_a_kept_rebuild_alone(ctx, files, tmp_path):
    import test_bam_reader as tbr
    import test_call_bam as tcb
    from cutesv_amd import extract, rebuild
    path = str(tmp_path / "edge.bam")
    tbr.write_edge(path)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    use = np.ones(ch.n, np.uint8)
    keys = ("ins_read", "ins_pos", "ins_len", "ins_piece0", "ins_npiece", "piece_qoff", "piece_len", "del_read", "del_pos", "del_len")
    grid, info = files["grid"]
    with _framed(ctx, grid, 2, index=False) as fb:
        cols = bam.decode(ctx, ch)
        want = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
        cols = bam.decode(ctx, ch)
        framed = fb.records("one", 0, 5000)
        assert framed.n > 0 and framed.valid()
        assert fb.build_index()["index_windows"] > 10 and fb.index_bytes() == info["bytes"]      # windows, framing kernels, index kernels
        assert not framed.valid()                                              # the build counts as a read: the device chunk is dead
        with pytest.raises(bam.BamError, match="device chunk is gone"):
            framed.slim
        got = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
        assert want["n_sig_ins"] > 100
        for k in keys:
            assert np.array_equal(got[k], want[k]), k
        seqs, rb = tcb.alt_pool(ctx)
        src = rb["src_row"]
        ins_rows = np.flatnonzero(src < len(tcb.ALT_LENS))
        clip = np.asarray([len(seqs[int(src[r])]) for r in ins_rows], np.int64)
        want = rebuild.alt_gather_host(seqs, src, ins_rows, clip)
        fb.build_index()
        got = rebuild.alt_gather(ctx, ins_rows, clip)
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and len(want[0]) > 1000
        assert fb.records("one", 0, 5000).n == framed.n                        # and the reader reads on, with its index
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
