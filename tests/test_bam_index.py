"""The BAM index of the native reader, on the CPU: the parser (cutesv_amd/csrc/bai_index.h) against an
independent writer (tests/bai_writer.py), the contract of an indexed read - THE INDEX ONLY MOVES THE STARTING POINT: the records
of a region, their order and both images are byte for byte those of the forward scan, and never more compressed bytes are read -
every refusal of a damaged index, the parser under the sanitizers, and the C ABI's additions."""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import bai_writer
import index_helpers as ih
from cutesv_amd import _abi, _lib, bam, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = bam.ALL


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    """the three-contig BAM with small blocks and its index -> (path, records, bai_writer's info)"""
    path = str(tmp_path_factory.mktemp("grid") / "grid.bam")
    recs, info = ih.write_grid_bam(path)
    return path, recs, info


# ------------------------------------------------------------------------------------ the fixture is what the issue asks for
def test_the_grid_bam_has_the_planted_shapes(grid):
    path, recs, info = grid
    assert len(info["blocks"]) >= 50 and [len(R["ioffset"]) for R in info["refs"]][1] == 0 and not info["refs"][1]["bins"]
    assert sum(1 for r in recs if r["refid"] >= 0) >= 400
    blocks = info["blocks"]
    ustart = np.r_[0, np.cumsum([b[2] for b in blocks])]
    inside = [r for r in info["records"] if np.searchsorted(ustart, r["off"], "right") != np.searchsorted(ustart, r["off_end"] - 1, "right")]
    assert inside, "no record straddles two blocks"
    assert sum(1 for r in info["records"] if r["off"] in set(ustart.tolist())) >= 3, "no record starts on a block boundary"
    assert sorted(r["end"] - r["pos"] for r in info["records"] if r["end"] - r["pos"] >= 20000) == [20000, 140000, 140000, 600000]
    assert any(r["flag"] & 4 and r["refid"] == 0 for r in info["records"]) and info["n_no_coor"] == 5


# ------------------------------------------------------------------------------------ parser against the writer
@pytest.mark.parametrize("variant", [dict(), dict(fill=False), dict(block_end=True), dict(pseudo=False), dict(no_coor=False)], ids=lambda v: "-".join(v) or "plain")
def test_statistics_and_n_no_coor_equal_the_writers(grid, tmp_path, variant):
    path, recs, _ = grid
    bai = str(tmp_path / "v.bai")
    info = bai_writer.write_bai(path, bai, **variant)
    if variant.get("block_end"):
        assert any(r["voff"] & 0xffff == b[2] for r in info["records"] for b in info["blocks"] if b[0] == r["voff"] >> 16 and b[2]), "no virtual offset at a block's end"
    with bam.BamFile(path, index=bai) as bf:
        assert bf.has_index
        want = [(name, R["n_mapped"], R["n_unmapped"], R["n_mapped"] + R["n_unmapped"]) for (name, _), R in zip(ih.REFS, info["refs"])]
        if variant.get("pseudo") is False:
            want = [(name, 0, 0, 0) for name, _ in ih.REFS]            # an index without the pseudo-bin reports zeros, as htslib does
        assert bf.index_statistics() == want
        assert bf.no_coordinate == (None if variant.get("no_coor") is False else 5)
        if not variant:
            assert [s[1] + s[2] for s in bf.index_statistics()] == [sum(1 for r in recs if r["refid"] == k) for k in range(3)]
            assert sum(s[2] for s in bf.index_statistics()) == 1


def test_an_index_beside_the_file_is_found_under_both_names(grid, tmp_path):
    path, _, info = grid
    for bam_name, bai_name in (("a.bam", "a.bam.bai"), ("b.bam", "b.bai")):
        shutil.copy(path, tmp_path / bam_name)
        (tmp_path / bai_name).write_bytes(info["bytes"])
        with bam.BamFile(str(tmp_path / bam_name)) as bf:
            assert bf.has_index
        with bam.BamFile(str(tmp_path / bam_name), index=False) as bf:
            assert not bf.has_index
            with pytest.raises(bam.BamError, match="no index"):
                bf.index_statistics()
    shutil.copy(path, tmp_path / "c.bam")
    with bam.BamFile(str(tmp_path / "c.bam")) as bf:                       # none beside it: fine, and none is loaded
        assert not bf.has_index
    with pytest.raises(bam.BamError, match="nowhere.bai"):
        bam.BamFile(str(tmp_path / "c.bam"), index=str(tmp_path / "nowhere.bai"))


# ------------------------------------------------------------------------------------ read grid
_pairs = ih.grid_pairs


def _fresh(bf):
    bf.set_inflate(None)                                                    # (drops the inflated window: every read pays for its own blocks)


@pytest.mark.parametrize("variant", [dict(), dict(fill=False), dict(block_end=True)], ids=lambda v: "-".join(v) or "plain")
def test_an_indexed_read_is_the_forward_scan_byte_for_byte(grid, tmp_path, variant):
    path, recs, _ = grid
    bai = str(tmp_path / "v.bai")
    info = bai_writer.write_bai(path, bai, **variant)
    n_checked = n_less = 0
    with bam.BamFile(path, index=bai) as ix, bam.BamFile(path, index=False) as fw:
        for chrom, (_, length), R in zip([r[0] for r in ih.REFS], ih.REFS, info["refs"]):
            pairs = list(_pairs(ih.grid_points(len(R["ioffset"]), length), length)) + [(-ALL, ALL), (0, length)]
            for beg, end in pairs:
                _fresh(ix); _fresh(fw)
                a, b = ix.records(chrom, beg, end), fw.records(chrom, beg, end)
                assert ih.same_chunk(a, b), (chrom, beg, end, a.n, b.n)
                want = [r["name"] for r in recs if r["refid"] == ix.refid(chrom) and r["start"] < end and r["start"] + max(sum(n for op, n in r["cigar"] if op in (0, 2, 3, 7, 8)), 1) > beg]
                assert [a.name(i) for i in range(a.n)] == want, (chrom, beg, end)
                assert a.stats["compressed_bytes"] <= b.stats["compressed_bytes"], (chrom, beg, end)
                n_less += a.stats["compressed_bytes"] < b.stats["compressed_bytes"]
                n_checked += 1
                if chrom == "none":
                    assert a.n == 0 and a.stats["compressed_bytes"] == 0          # a reference without records: no block is touched
        assert n_checked > 300 and n_less > 100
        # a region on the last contig: strictly fewer compressed bytes, from a reader that has seen nothing yet
    with bam.BamFile(path, index=bai) as ix, bam.BamFile(path, index=False) as fw:
        a, b = ix.records("two", 20 * ih.WINDOW, 21 * ih.WINDOW), fw.records("two", 20 * ih.WINDOW, 21 * ih.WINDOW)
        assert ih.same_chunk(a, b) and a.n > 0 and 0 < a.stats["compressed_bytes"] < b.stats["compressed_bytes"]
        # behind n_intv: nothing overlaps, nothing is read
        a = ix.records("two", 50 * ih.WINDOW, ALL)
        assert a.n == 0 and a.stats["compressed_bytes"] == 0


def test_chunked_reads_and_counts_do_not_depend_on_the_index(grid):
    path, recs, _ = grid
    with bam.BamFile(path) as ix, bam.BamFile(path, index=False) as fw:
        assert ix.has_index
        for chrom in ("one", "none", "two", None):
            assert ix.count(chrom) == fw.count(chrom) == sum(1 for r in recs if r["refid"] == ix.refid(chrom))
            for kw in (dict(), dict(start=2 * ih.WINDOW - 1, end=30 * ih.WINDOW + 1)):
                if chrom is None and kw:
                    continue
                ca, cb = list(ix.chunks(chrom, chunk_records=7, **kw)), list(fw.chunks(chrom, chunk_records=7, **kw))
                assert len(ca) == len(cb) and all(ih.same_chunk(x, y) for x, y in zip(ca, cb))
        # the index is dropped: the reader goes on as one that never had it, whatever the indexed reads left behind
        ix.records("two", 20 * ih.WINDOW, 21 * ih.WINDOW)
        ix.drop_index()
        assert not ix.has_index
        for chrom in ("two", "one", None):
            assert ih.same_chunk(ix.records(chrom, -ALL, ALL), fw.records(chrom, -ALL, ALL))


def _union(bf, chrom, ranges):
    """the single reads of the ranges, concatenated with duplicates removed (a record is known by where its slim image came from:
    its name and start) - in file order"""
    seen, names = set(), []
    for beg, end in ranges:
        ch = bf.records(chrom, beg, end)
        for i in range(ch.n):
            key = (ch.name(i), int(ch.slim[int(ch.rec_off[i]) + 4 : int(ch.rec_off[i]) + 8].view(np.int32)[0]))
            if key not in seen:
                seen.add(key); names.append(key)
    return names


def test_multi_range_reads(grid):
    path, recs, info = grid
    W = ih.WINDOW
    cases = [[(0, 10)], [(0, W - 1), (W - 1, W), (W, W + 1)], [(5, 900), (2 * W - 3, 2 * W + 50), (12 * W - 90, 12 * W), (44 * W, 46 * W)],
             [(3 * W + 100, 3 * W + 200), (7 * W, 8 * W), (30 * W + 5000, 30 * W + 5100)], [(0, 0), (0, 5), (5, 5), (6, 7)], [(200_000, 200_200), (340_100, 340_101), (601_000, 700_000)],
             [(50 * W, 60 * W), (70 * W, ALL)], [(-ALL, 100), (20 * W, ALL)]]
    with bam.BamFile(path) as ix, bam.BamFile(path, index=False) as fw:
        for chrom in ("one", "two", "none"):
            for ranges in cases:
                _fresh(ix); _fresh(fw)
                a, b = ix.records(chrom, ranges=ranges), fw.records(chrom, ranges=ranges)
                assert ih.same_chunk(a, b), (chrom, ranges)
                got = [(a.name(i), int(a.slim[int(a.rec_off[i]) + 4 : int(a.rec_off[i]) + 8].view(np.int32)[0])) for i in range(a.n)]
                want = _union(fw, chrom, ranges)
                assert sorted(got, key=lambda t: t[1]) == sorted(want, key=lambda t: t[1]) and len(set(got)) == len(got), (chrom, ranges)
                assert [t[1] for t in got] == sorted(t[1] for t in got)                     # file order
                assert a.stats["compressed_bytes"] <= b.stats["compressed_bytes"]
                ca, cb = list(ix.chunks(chrom, chunk_records=3, ranges=ranges)), list(fw.chunks(chrom, chunk_records=3, ranges=ranges))
                assert sum(c.n for c in ca) == a.n and len(ca) == len(cb) and all(ih.same_chunk(x, y) for x, y in zip(ca, cb))
        _fresh(ix); _fresh(fw)
        far = [(5, 900), (44 * W, 46 * W)]
        assert ix.records("one", ranges=far).stats["compressed_bytes"] < fw.records("one", ranges=far).stats["compressed_bytes"]
        assert ix.records("one", ranges=[]).n == 0 and ix.last_stats["compressed_bytes"] == 0
        for bad in ([(5, 4)], [(0, 10), (9, 20)], [(20, 30), (0, 10)]):
            with pytest.raises(ValueError):
                ix.records("one", ranges=bad)
    L = _lib.lib()
    with bam.BamFile(path) as bf:                                             # the entry refuses them itself as well
        beg, end, cc = np.array([0, 9], np.int64), np.array([10, 20], np.int64), _abi.ChunkC()
        assert L.csv_bam_read_ranges(bf._h, 0, 2, beg.ctypes.data, end.ctypes.data, 10, _abi.BAM_RESTART, cc) == _abi.E_INVALID
        assert L.csv_bam_read_ranges(bf._h, 0, 0, beg.ctypes.data, end.ctypes.data, 10, _abi.BAM_RESTART, cc) == _abi.E_INVALID


# ------------------------------------------------------------------------------------ refusals
def _damaged(info):
    """[(what, bytes)] - every one must be refused: cut at every byte position (but the one in front of the optional n_no_coor,
    which leaves a well-formed index), and each count field set to -1 and 2^31 - 1"""
    data = info["bytes"]
    fo = bai_writer.field_offsets(data)
    assert fo["end_refs"] == len(data) - 8
    out = [("cut at %d" % k, data[:k]) for k in range(len(data)) if k != fo["end_refs"]]
    for field in ("n_bin", "n_chunk", "n_intv"):
        for off in fo[field]:
            for v in (-1, 2 ** 31 - 1):
                out.append(("%s at %d = %d" % (field, off, v), data[:off] + struct.pack("<i", v) + data[off + 4:]))
    for v in (-1, 2 ** 31 - 1):
        out.append(("n_ref = %d" % v, data[:4] + struct.pack("<i", v) + data[8:]))
    return out, fo


def test_every_damaged_index_is_refused_with_a_text_that_names_it(grid, tmp_path):
    path, _, info = grid
    damaged, fo = _damaged(info)
    bai = str(tmp_path / "damaged.bai")
    L = _lib.lib()
    with bam.BamFile(path, index=False) as bf:
        for what, data in damaged:
            with open(bai, "wb") as f:
                f.write(data)
            assert L.csv_bam_index_load(bf._h, os.fsencode(bai)) == _abi.E_INVALID, what
            assert b"damaged.bai" in L.csv_bam_error(bf._h), what
        assert not bf.has_index
        with open(bai, "wb") as f:                                             # the one cut that leaves a well-formed index: no n_no_coor
            f.write(info["bytes"][:fo["end_refs"]])
        assert bf.load_index(bai) and bf.no_coordinate is None


def _with(data, off, fmt, value):
    return data[:off] + struct.pack(fmt, value) + data[off + struct.calcsize(fmt):]


def test_the_checks_of_the_parser_one_by_one(grid, tmp_path):
    path, _, info = grid
    data = info["bytes"]
    fo = bai_writer.field_offsets(data)
    io_off, n_intv = fo["ioffset"][0]
    assert n_intv > 10
    v5, = struct.unpack_from("<Q", data, io_off + 8 * 5)
    blocks = info["blocks"]
    mid = next(b for b in blocks if b[2] > 0 and b[0] > 0)
    cases = [
        ("magic", b"BAI\2" + data[4:], "magic"),
        ("n_ref of another file", _with(data, 4, "<i", 2), "the BAM header has"),
        ("n_ref of another file, whole", bai_writer.to_bytes(dict(n_ref=2, refs=info["refs"][:2], n_no_coor=0)), "the BAM header has"),
        ("negative n_bin", _with(data, fo["n_bin"][0], "<i", -7), "negative n_bin"),
        ("absurd n_bin", _with(data, fo["n_bin"][0], "<i", 10 ** 6), "absurd n_bin"),
        ("negative n_chunk", _with(data, fo["n_chunk"][0], "<i", -1), "negative n_chunk"),
        ("absurd n_chunk", _with(data, fo["n_chunk"][0], "<i", 2 ** 31 - 1), "absurd n_chunk"),
        ("negative n_intv", _with(data, fo["n_intv"][0], "<i", -1), "negative n_intv"),
        ("absurd n_intv", _with(data, fo["n_intv"][0], "<i", 2 ** 30), "absurd n_intv"),
        ("ends inside the linear index", data[: io_off + 12], "ends inside"),
        ("decreasing linear index", _with(data, io_off + 8 * 5, "<Q", struct.unpack_from("<Q", data, io_off + 8 * 30)[0] + 1), "decreases"),
        ("coffset inside a block", _with(data, io_off + 8 * 5, "<Q", ((v5 >> 16) + 1) << 16 | (v5 & 0xffff)), "not the start of a BGZF block"),
        ("coffset behind the file", _with(data, io_off + 8 * (n_intv - 1), "<Q", (blocks[-1][0] + blocks[-1][1] + 9) << 16), "not the start of a BGZF block"),
        ("uoffset above ISIZE", _with(data, io_off + 8 * 5, "<Q", (v5 >> 16) << 16 | 0xffff), "above its ISIZE"),
        ("chunk coffset inside a block", _with(data, fo["n_chunk"][0] + 4, "<Q", (mid[0] + 1) << 16), "not the start of a BGZF block"),
    ]
    bai = str(tmp_path / "one_check.bai")
    for what, bad, text in cases:
        with open(bai, "wb") as f:
            f.write(bad)
        with pytest.raises(bam.BamError, match="one_check.bai.*" + re.escape(text)):
            bam.BamFile(path, index=bai)
    # ... and found beside the file it is no less an error: an invalid index is never skipped in silence
    shutil.copy(path, tmp_path / "x.bam")
    (tmp_path / "x.bam.bai").write_bytes(cases[0][1])
    with pytest.raises(bam.BamError, match="x.bam.bai"):
        bam.BamFile(str(tmp_path / "x.bam"))
    with bam.BamFile(str(tmp_path / "x.bam"), index=False) as bf:
        assert bf.count("two") > 0


def test_task_cut_index_needs_an_index(grid):
    path, _, _ = grid
    with bam.BamFile(path, index=False) as bf:
        with pytest.raises(ValueError, match="index"):
            call.call_bam(bf, {}, call.CallParams(), ctx=object(), task_cut="index")
        with pytest.raises(ValueError, match="task_cut"):
            call.call_bam(bf, {}, call.CallParams(), ctx=object(), task_cut="even")


# ------------------------------------------------------------------------------------ the parser under the sanitizers
def test_the_parser_under_the_sanitizers_equals_the_library(grid, tmp_path):
    """bai_index.h in a stand-alone program built with -fsanitize=address,undefined over the damaged indexes (and the sound ones): each
    file is a heap block of exactly its size there, so a read behind a file that ends inside a field ends the program.  The
    sanitizers' runtimes are linked into it; nothing is preloaded."""
    path, _, info = grid
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (the library's own build needs it too)"
    exe, corpus = str(tmp_path / "bai_parse_main"), str(tmp_path / "corpus.bin")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "bai_parse_main.cpp")], check=True, capture_output=True, text=True)
    damaged, fo = _damaged(info)
    sound = [("whole", info["bytes"]), ("no n_no_coor", info["bytes"][:fo["end_refs"]]), ("zeros", bai_writer.write_bai(path, str(tmp_path / "z.bai"), fill=False)["bytes"]),
             ("no pseudo-bin", bai_writer.write_bai(path, str(tmp_path / "p.bai"), pseudo=False)["bytes"])]
    files = damaged + sound
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for _, data in files:
            f.write(struct.pack("<I", len(data)) + data)
    p = subprocess.run([exe, corpus, "3"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = [[int(x) for x in ln.split()] for ln in p.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(len(files)))
    assert all(r[1] == 0 for r in rows[:len(damaged)]), [files[r[0]][0] for r in rows[:len(damaged)] if r[1]][:5]
    n_intv = sum(len(R["ioffset"]) for R in info["refs"])
    mapped, unmapped = sum(R["n_mapped"] for R in info["refs"]), sum(R["n_unmapped"] for R in info["refs"])
    first = info["refs"][0]["ioffset"][0]
    assert rows[len(damaged):] == [[len(damaged), 1, 3, n_intv, mapped, unmapped, 5, first], [len(damaged) + 1, 1, 3, n_intv, mapped, unmapped, -1, first],
                                   [len(damaged) + 2, 1, 3, n_intv, mapped, unmapped, 5, first], [len(damaged) + 3, 1, 3, n_intv, 0, 0, 5, first]]


# ------------------------------------------------------------------------------------ ABI
def test_the_header_declares_what_the_library_exports_and_the_abi_is_9():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define CSV_ABI_VERSION 9\b", text) and _abi.ABI_VERSION == 9 and _lib.lib().csv_abi_version() == 9
    declared = set(re.findall(r"^[A-Za-z_][\w \t\*]*?\b(csv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    new = {"csv_bam_index_load", "csv_bam_index_drop", "csv_bam_index_stats", "csv_bam_read_ranges"}
    assert new <= declared and new <= bound
    assert bound <= declared, sorted(bound - declared)
    nm = shutil.which("nm")
    if nm:                                                                     # what the library exports under the prefix is what the header declares
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("csv_") and ln.split()[-2] in "TW"}
        assert new <= exported and exported <= declared, sorted(exported - declared)
    L = _lib.lib()
    assert [L.csv_bam_struct_size(i) for i in range(4)] == [s for _, s in _abi.BAM_STRUCT_SIZES] + [-1]


def test_idxstats_command_line(grid):
    path, _, info = grid
    p = subprocess.run([sys.executable, "-m", "cutesv_amd.bam", path, "--idxstats"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    want = ["%s\t%d\t%d\t%d" % (n, ln, R["n_mapped"], R["n_unmapped"]) for (n, ln), R in zip(ih.REFS, info["refs"])] + ["*\t0\t0\t5"]
    assert p.stdout.splitlines() == want


# ------------------------------------------------------------------------------------ the reference's cut
def test_cut_tasks_index_and_for_task_equal_the_reference_bit_for_bit():
    import gzip
    import json
    from cutesv_amd import bed
    with gzip.open(os.path.join(ROOT, "tests", "golden", "index_cut.json.gz"), "rt") as f:
        cases = json.load(f)
    assert {c["threads"] for c in cases} >= {1, 16, 64}
    slivers = fractional = 0
    for c in cases:
        got = call.cut_tasks_index([tuple(s) for s in c["stats"]], c["lengths"], c["batch"], c["threads"])
        assert len(got) == len(c["tasks"]), c["name"]
        for (gc, g0, g1), (wc, w0, w1) in zip(got, c["tasks"]):
            assert gc == wc and type(g0) is type(w0) and type(g1) is type(w1), (c["name"], gc, g0, g1)
            assert float(g0).hex() == float(w0).hex() and float(g1).hex() == float(w1).hex(), (c["name"], gc, g0, w0, g1, w1)
            slivers += 0 < g1 - g0 < 1
            fractional += g0 != int(g0)
        regions = bed.Regions.from_intervals({k: [tuple(x) for x in v] for k, v in c["bed"].items()})
        for (gc, g0, g1), want in zip(got, c["regions"]):
            assert regions.for_task(gc, g0, g1).tolist() == want, (c["name"], gc, g0, g1)
            i0, i1 = call.task_bounds(g0, g1)
            assert all((s >= g0) == (s >= i0) and (s < g1) == (s < i1) for s in (int(g0) - 1, int(g0), int(g0) + 1, int(g1) - 1, int(g1), int(g1) + 1))
    assert slivers >= 2 and fractional > 10
    assert any(want for c in cases for want in c["regions"])


# ------------------------------------------------------------------------------------ what one read leaves behind for the next
@pytest.mark.parametrize("index", [None, False], ids=["indexed", "forward"])
def test_reads_of_one_reader_interleaved_equal_those_of_fresh_readers(grid, index):
    """the region hint, the contig starts and the kept window across multi-range and single reads of ONE reader, nothing dropped
    in between: every read equals the same read of a reader that has seen nothing"""
    path, _, _ = grid
    W = ih.WINDOW
    reads = [("two", [(13 * W, 14 * W), (40 * W, 41 * W)]), ("two", (20 * W, 21 * W)), ("two", (12 * W, 13 * W)), ("one", [(5, 900), (44 * W, 46 * W)]), ("one", (20 * W, 21 * W)),
             ("one", (30 * W, ALL)), ("one", [(0, 10), (12 * W - 90, 12 * W), (30 * W + 5000, 30 * W + 5100)]), ("one", (12 * W, 13 * W)), ("two", [(0, 5), (9 * W, 9 * W + 50)]),
             ("two", (5 * W - 1, 5 * W + 100)), ("two", (3 * W, 4 * W)), ("two", (-ALL, ALL)), ("one", (-ALL, ALL)), (None, (-ALL, ALL))]

    def read(bf, chrom, what):
        return bf.records(chrom, ranges=what) if isinstance(what, list) else bf.records(chrom, *what)
    with bam.BamFile(path, index=index) as one:
        for chrom, what in reads:
            with bam.BamFile(path, index=False) as fresh:
                a, b = read(one, chrom, what), read(fresh, chrom, what)
            assert ih.same_chunk(a, b) and (a.n > 0 or chrom == "two" and what == (3 * W, 4 * W)), (chrom, what, a.n, b.n)


def test_a_dropped_index_leaves_nothing_behind(grid):
    """two indexed reads of overlapping regions (the second starts at the first's hint), then the index is dropped: the forward scan
    of the whole contig - and of the one in front, and of the tail - finds every record"""
    path, recs, _ = grid
    W = ih.WINDOW
    with bam.BamFile(path) as bf, bam.BamFile(path, index=False) as fw:
        for region in ((20 * W, 21 * W), (20 * W, 21 * W), (20 * W + 100, 30 * W)):
            assert ih.same_chunk(bf.records("two", *region), fw.records("two", *region))
        bf.drop_index()
        for chrom in ("two", "one", None, "two"):
            a = bf.records(chrom, -ALL, ALL)
            assert a.n == sum(1 for r in recs if r["refid"] == bf.refid(chrom)) and ih.same_chunk(a, fw.records(chrom, -ALL, ALL)), chrom


def test_a_failed_load_leaves_no_index_on_either_side(grid, tmp_path):
    path, _, info = grid
    bad = str(tmp_path / "bad.bai")
    with open(bad, "wb") as f:
        f.write(info["bytes"][:-20])
    with bam.BamFile(path) as bf:
        assert bf.has_index
        with pytest.raises(bam.BamError, match="bad.bai"):
            bf.load_index(bad)
        assert not bf.has_index
        assert _lib.lib().csv_bam_index_stats(bf._h, None, None, None) == _abi.E_STATE and _lib.lib().csv_bam_index_block(bf._h, 0, 0) == -2
        with bam.BamFile(path, index=False) as fw:
            assert ih.same_chunk(bf.records("two", 20 * ih.WINDOW, 21 * ih.WINDOW), fw.records("two", 20 * ih.WINDOW, 21 * ih.WINDOW))
            assert bf.last_stats["compressed_bytes"] == fw.last_stats["compressed_bytes"]
