"""The CSI index on the host: the parser (csrc/csi_index.h) against tests/csi_writer.py - an independent writer
from the format's text - on the files of the BAI build tests at (14, 5), on a two-contig file with contigs of 600 Mbp at (14, 6) and on
a file at (12, 6); one crafted file per refusal; the built index against bai_writer's at (14, 5) and against csi_writer's bytes; the
.csi file's BGZF form; the read grid on the 600 Mbp file; the statistics and the task cut; the discovery order; and, under the
sanitizers, the parser and bytes_csi() alone (tests/csi_core_main.cpp)."""
import bisect
import gzip
import os
import shutil
import struct
import subprocess

import pytest

import bai_writer
import csi_helpers as ch
import csi_writer as cw
import index_build_helpers as H
import index_helpers as ih
from cutesv_amd import bam, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 1 << 62


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """{name: path} of the files of the BAI build tests"""
    d = tmp_path_factory.mktemp("csi_small")
    return dict(H.parity_files(d))


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """the 600 Mbp file -> (path, its records, csi_writer's info at htslib's scheme (14, 6), the .csi path)"""
    d = tmp_path_factory.mktemp("csi_big")
    path = str(d / "big.bam")
    recs = ch.write_big(path)
    info = cw.write_csi(path, str(d / "big.csi.keep"))
    assert (info["min_shift"], info["depth"]) == (14, 6)
    return path, recs, info, info["path"]


def _block_of(info, voff):
    return [b[0] for b in info["blocks"]].index(voff >> 16)


def _expected_start(info, refid, beg):
    """the format's rule, from the writer's own tables: the loffset of the bin with the greatest first base <= beg; else the first record"""
    R = info["refs"][refid]
    if not R["bins"]:
        return None
    table = {}
    for b, lo in R["loff"].items():
        base = cw.bot(b, info["depth"]) << info["min_shift"]
        if lo:
            table[base] = min(lo, table.get(base, lo))
    bases = sorted(table)
    k = bisect.bisect_right(bases, max(beg, 0))
    return table[bases[k - 1]] if k else R["beg"]


def _check_against_writer(path, info, csi_path, points):
    with bam.BamFile(path, index=csi_path) as bf:
        assert bf.has_index and bf.index_format == "csi"
        want = [(n, R["n_mapped"], R["n_unmapped"], R["n_mapped"] + R["n_unmapped"]) for n, R in zip(bf.references, info["refs"])]
        assert bf.index_statistics() == want and bf.no_coordinate == info["n_no_coor"]
        for refid, name in enumerate(bf.references):
            for p in points:
                v = _expected_start(info, refid, p)
                assert bf.index_block(name, p) == (-1 if v is None else _block_of(info, v)), (name, p)


# ------------------------------------------------------------------------------------------------ the parser against the writer
def test_a_csi_is_loaded_and_read_as_the_writer_wrote_it_at_14_5(small, tmp_path):
    for name, path in small.items():
        info = cw.write_csi(path, str(tmp_path / (name + ".csi")), 14, 5)
        pts = [0, 1, 16383, 16384, 3 * 16384 - 1, 5 * 16384, 100_000, 131072, 300_000, 700_000, 1 << 20, 1_999_999, 1 << 28, (1 << 29) - 1]
        _check_against_writer(path, info, info["path"], pts)


def test_a_600_mbp_file_at_14_6_and_at_12_6(big, tmp_path):
    path, recs, info, csi = big
    assert max(r["start"] for r in recs) == ch.L600 - 1 and sum(1 for r in recs if r.get("refid", 0) == 0 and r["start"] >= ch.P29) > 200
    _check_against_writer(path, info, csi, ch.big_points())
    other = cw.write_csi(path, str(tmp_path / "b12.csi"), 12, 6)
    assert other["payload"] != info["payload"]
    _check_against_writer(path, other, other["path"], ch.big_points())
    # several BGZF blocks in the index file itself
    blocks = cw.write_csi(path, str(tmp_path / "blocks.csi"), block_bytes=100)
    assert blocks["bytes"].count(b"\x1f\x8b\x08\x04") > 5
    _check_against_writer(path, blocks, blocks["path"], ch.big_points()[:8])


# ------------------------------------------------------------------------------------------------ one crafted file per refusal
def _put(payload, off, fmt, *values):
    b = bytearray(payload)
    struct.pack_into(fmt, b, off, *values)
    return bytes(b)


def test_every_refusal_of_the_parser_with_its_text(big, small, tmp_path):
    path, _, info, _ = big
    p = info["payload"]
    f = cw.fields(p)
    regular = [b for b in f["bins"] if b["bin"] != cw.pseudo_bin(6)]
    pseudo = [b for b in f["bins"] if b["bin"] == cw.pseudo_bin(6)]
    a_bin = regular[3]
    first_chunk = struct.unpack_from("<QQ", p, a_bin["chunks_at"])
    bad_voff = (info["blocks"][5][0] + 1) << 16
    # two bins of one reference whose first bases ascend: the later one gets a loffset below the earlier one's
    by_base = sorted(((cw.bot(b["bin"], 6), b["loffset"], b) for b in regular if b["ref"] == 0 and b["loffset"]), key=lambda x: x[:2])
    later = next(x for x in by_base if x[0] > by_base[0][0] and x[1] > by_base[0][1])
    cases = [
        ("magic", b"CSJ\1" + p[4:], "no CSI\\\\1 magic"),
        ("n_ref", _put(p, f["n_ref_at"], "<i", 3), "the index has 3 references, the BAM header has"),
        ("neg_n_ref", _put(p, f["n_ref_at"], "<i", -1), "negative n_ref"),
        ("neg_n_bin", _put(p, f["n_bin_at"][0], "<i", -2), "negative n_bin"),
        ("absurd_n_bin", _put(p, f["n_bin_at"][0], "<i", 1 << 30), "absurd n_bin"),
        ("neg_n_chunk", _put(p, a_bin["at"] + 12, "<i", -1), "negative n_chunk"),
        ("absurd_n_chunk", _put(p, a_bin["at"] + 12, "<i", (1 << 28) + 1), "absurd n_chunk"),
        ("min_shift", _put(p, 4, "<i", 0), "min_shift below 1"),
        ("depth", _put(p, 8, "<i", -1), "negative depth"),
        ("too_deep", _put(p, 4, "<ii", 40, 8), "min_shift \\+ 3 \\* depth above 62"),
        ("l_aux", _put(p, 12, "<i", -4), "negative l_aux"),
        ("bin", _put(p, a_bin["at"], "<I", cw.pseudo_bin(6) + 1), "bin number out of range"),
        ("pseudo_chunks", p[: pseudo[-1]["at"] + 12] + struct.pack("<i", 1) + p[pseudo[-1]["at"] + 16 : pseudo[-1]["at"] + 32] + p[pseudo[-1]["at"] + 48 :],
         "the pseudo-bin 299594 needs two chunks, found"),
        ("chunk_order", _put(p, a_bin["chunks_at"], "<QQ", first_chunk[1], first_chunk[0] - 1 if first_chunk[0] == first_chunk[1] else first_chunk[0]), "a chunk ends before it begins"),
        ("truncated", p[: a_bin["chunks_at"] + 5], "the file ends inside a bin's chunks"),
        ("truncated_header", p[:10], "the file ends inside min_shift, depth and l_aux"),
        ("truncated_tail", p[:-3], "the file ends inside n_no_coor"),
        ("coffset", _put(p, a_bin["chunks_at"], "<Q", bad_voff), "is not the start of a BGZF block of the BAM file"),
        ("uoffset", _put(p, a_bin["chunks_at"] + 8, "<Q", first_chunk[1] | 0xFFFF), "is above its ISIZE"),
        ("loffset_voff", _put(p, a_bin["at"] + 4, "<Q", bad_voff - (2 << 16)) if bad_voff - (2 << 16) <= first_chunk[0] else None, "loffset: coffset"),
        ("loffset_behind", _put(p, a_bin["at"] + 4, "<Q", first_chunk[1]) if first_chunk[1] > first_chunk[0] else None, "the loffset lies behind a chunk of its own bin"),
        ("loffset_decreases", _put(p, later[2]["at"] + 4, "<Q", info["refs"][0]["beg"]) if by_base[0][1] > info["refs"][0]["beg"] else None, "the loffset decreases at base"),
    ]
    n = 0
    for what, payload, text in cases:
        if payload is None:
            continue
        n += 1
        bad = cw.write_payload(tmp_path / (what + ".csi"), payload)
        with bam.BamFile(path, index=False) as bf:
            with pytest.raises(bam.BamError, match=text) as ei:
                bf.load_index(bad)
            assert what + ".csi" in str(ei.value) and not bf.has_index and bf.index_format is None, what
    assert n >= 20
    # the file's own damage: no end-of-file block; a block that does not inflate
    with bam.BamFile(path, index=False) as bf:
        with pytest.raises(bam.BamError, match="noeof.csi: the BGZF end-of-file block is missing"):
            bf.load_index(cw.write_payload(tmp_path / "noeof.csi", p, eof=False))
        blob = bytearray(cw.compress(p))
        blob[40] ^= 0x55
        (tmp_path / "flip.csi").write_bytes(bytes(blob))
        with pytest.raises(bam.BamError, match="flip.csi"):
            bf.load_index(str(tmp_path / "flip.csi"))
        assert not bf.has_index


# ------------------------------------------------------------------------------------------------ equivalence with the BAI build
def test_at_14_5_the_built_csi_is_the_bai_with_loffsets(small):
    for name, path in small.items():
        twin = H.twin(path)
        with bam.BamFile(path, index=False) as bf:
            st = bf.build_index(format="csi", depth=5)
            got = cw.read_payload(bf.index_payload())
            assert st["format"] == "csi" and bf.index_format == "csi" and (got["min_shift"], got["depth"]) == (14, 5)
            assert H.same_stats(bf, twin, bf.references)
        assert got["n_no_coor"] == twin["n_no_coor"]
        for R, T in zip(got["refs"], twin["refs"]):
            assert {b: list(c) for b, (_, c) in R["bins"].items()} == {b: list(c) for b, c in T["bins"].items()}, name
            assert R["order"] == sorted(T["bins"]) + ([37450] if T["beg"] is not None else []), name          # bins ascending, the pseudo-bin last
            assert R["pseudo"] == (None if T["beg"] is None else (T["beg"], T["end"], T["n_mapped"], T["n_unmapped"])), name
            for b, (lo, _) in R["bins"].items():
                assert lo == T["ioffset"][cw.bot(b, 5)] != 0, (name, b)                                       # the filled linear entry


def test_the_host_build_equals_the_writer_byte_for_byte(small, big, tmp_path):
    cases = [(p, 14, None) for p in small.values()] + [(p, 14, 5) for p in list(small.values())[:6]] + [(big[0], 14, None), (big[0], 14, 6), (big[0], 12, 6), (big[0], 15, 6), (big[0], 14, 7)]
    for path, min_shift, depth in cases:
        want = cw.write_csi(path, str(tmp_path / "w.csi"), min_shift, depth)
        with bam.BamFile(path, index=False) as bf:
            st = bf.build_index(format="csi", min_shift=min_shift, depth=depth)
            assert bf.index_payload() == want["payload"], (path, min_shift, depth)
            data = bf.index_bytes()
            assert st["index_bytes"] == len(data) and st["bytes_down"] == 0 and st["records"] == len(want["records"])
        # the .csi file: gzip members that inflate to the payload, the BGZF end-of-file block last; the independent walk reads it too
        assert gzip.decompress(data) == want["payload"] and data.endswith(cw.EOF_BLOCK)
        assert b"".join([bai_writer.read_blocks(data)[1]]) == want["payload"]
    with bam.BamFile(big[0], index=False) as bf:                               # htslib's rule for the depth
        bf.build_index(format="csi")
        assert cw.read_payload(bf.index_payload())["depth"] == 6
    with bam.BamFile(list(small.values())[0], index=False) as bf:
        bf.build_index(format="csi")
        assert cw.read_payload(bf.index_payload())["depth"] == 3                # 2 000 000 + 256 <= 2^(14 + 9)
        bf.build_index()                                                        # a BAI build afterwards: the reader's index is a .bai again
        assert bf.index_format == "bai" and bf.index_bytes()[:4] == b"BAI\1"
        with pytest.raises(bam.BamError, match="no built CSI index"):
            bf.index_payload()


def test_write_goes_to_the_csi_name_and_the_file_loads(big, tmp_path):
    path = str(tmp_path / "w.bam")
    shutil.copy(big[0], path)
    with bam.BamFile(path, index=False) as bf:
        st = bf.build_index(write=True, format="csi")
        assert st["written"] == path + ".csi" and open(path + ".csi", "rb").read() == bf.index_bytes()
        with pytest.raises(FileExistsError):
            bf.build_index(write=True, format="csi")
    with bam.BamFile(path) as bf:
        assert bf.index_format == "csi" and bf.index_statistics()[0][3] > 300
    out = str(tmp_path / "cli.csi")
    assert bam.main([path, "--index", "--csi", "--index_out", out]) == 0 and open(out, "rb").read() == open(path + ".csi", "rb").read()
    assert bam.main([path, "--index", "--csi", "--min_shift", "12", "--index_out", out, "--force"]) == 0
    assert cw.read_payload(gzip.decompress(open(out, "rb").read()))["min_shift"] == 12
    with pytest.raises(SystemExit):
        bam.main([path, "--csi"])
    assert bam.main([path, "--idxstats"]) == 0


def test_refusals_of_a_csi_build_on_the_host(tmp_path):
    for name, (refs, recs, (min_shift, depth), ordinal, text) in ch.REFUSALS.items():
        path = str(tmp_path / (name + ".bam"))
        ch.write_bam(path, refs, recs, block_bytes=300)
        with bam.BamFile(path, index=False) as bf:
            with pytest.raises(bam.BamError) as ei:
                bf.build_index(format="csi", min_shift=min_shift, depth=depth, write=True)
            assert "cannot build the index: record %d %s" % (ordinal, text) in str(ei.value) and not bf.has_index, name
        assert os.listdir(tmp_path).count(name + ".bam.csi") == 0
    # a BAI build of a file that needs CSI: today's refusal, and one sentence that names the way out
    with bam.BamFile(str(tmp_path / "beyond_max_pos.bam"), index=False) as bf:
        with pytest.raises(bam.BamError, match="reaches 2\\^29 bases or beyond, which the BAI format cannot index.*format=\"csi\""):
            bf.build_index()
        for kw in (dict(min_shift=3), dict(min_shift=40), dict(depth=-1), dict(min_shift=20, depth=15), dict(min_shift=4, depth=9)):
            with pytest.raises(bam.BamError, match="cannot build the index: min_shift"):
                bf.build_index(format="csi", **kw)
        with pytest.raises(ValueError):
            bf.build_index(format="tbi")


# ------------------------------------------------------------------------------------------------ the read grid
_fresh, check_read_grid = ch.fresh, ch.check_read_grid


def test_an_indexed_read_on_the_600_mbp_file_is_the_forward_scan(big):
    path, recs, _, csi = big
    with bam.BamFile(path, index=csi) as ix, bam.BamFile(path, index=False) as fw:
        check_read_grid(ix, fw, recs)
        # multi-range reads jump between the ranges
        ranges = [(100, 200), (ch.P29 - 1, ch.P29 + 5), (580_000_000, 580_000_100)]
        _fresh(ix); _fresh(fw)
        a, b = ix.records("also", ranges=ranges), fw.records("also", ranges=ranges)
        assert ih.same_chunk(a, b) and a.n >= 5 and a.stats["compressed_bytes"] < b.stats["compressed_bytes"]
    with bam.BamFile(path, index=csi) as ix, bam.BamFile(path, index=False) as fw:
        a, b = ix.records("also", 580_000_000, 580_000_001), fw.records("also", 580_000_000, 580_000_001)
        assert ih.same_chunk(a, b) and a.n == 1 and 0 < a.stats["compressed_bytes"] < b.stats["compressed_bytes"] / 4      # a direct seek


def test_an_empty_reference_touches_no_block(small, tmp_path):
    path = small["grid"]
    info = cw.write_csi(path, str(tmp_path / "g.csi"))
    with bam.BamFile(path, index=info["path"]) as bf:
        a = bf.records("none", 0, ALL)
        assert a.n == 0 and a.stats["compressed_bytes"] == 0 and bf.index_block("none", 0) == -1


# ------------------------------------------------------------------------------------------------ statistics, the cut, discovery
def test_statistics_and_the_index_cut_equal_those_of_the_bai(small, tmp_path):
    path = str(tmp_path / "g.bam")
    shutil.copy(small["grid"], path)
    csi = cw.write_csi(path, str(tmp_path / "only.csi"))
    bai = bai_writer.write_bai(path, str(tmp_path / "only.bai"))
    with bam.BamFile(path, index=csi["path"]) as c, bam.BamFile(path, index=bai["path"]) as b:
        assert (c.index_format, b.index_format) == ("csi", "bai")
        assert c.index_statistics() == b.index_statistics() and c.no_coordinate == b.no_coordinate and sum(s[3] for s in c.index_statistics()) > 400
        length = dict(zip(c.references, c.lengths))
        for batch, threads in ((10_000_000, 16), (100_000, 4), (30_000, 1)):
            assert call.cut_tasks_index(c.index_statistics(), length, batch, threads) == call.cut_tasks_index(b.index_statistics(), length, batch, threads)
        for chrom in c.references:
            for beg in (0, 16384, 5 * 16384 + 3, 700_000):
                _fresh(c); _fresh(b)
                assert ih.same_chunk(c.records(chrom, beg, beg + 40_000), b.records(chrom, beg, beg + 40_000))


def test_the_discovery_order(small, tmp_path):
    src = small["grid"]
    csi = cw.write_csi(src, str(tmp_path / "src.csi"))["bytes"]
    bai = bai_writer.write_bai(src, str(tmp_path / "src.bai"))["bytes"]
    d = tmp_path / "d"
    d.mkdir()
    bam_path = str(d / "x.bam")
    shutil.copy(src, bam_path)
    names = ["x.bam.bai", "x.bai", "x.bam.csi", "x.csi"]
    fmt = lambda: bam.BamFile(bam_path).index_format                             # noqa: E731
    assert fmt() is None
    # from the last candidate to the first: each one, once present, wins over those behind it.  The content is the other format's
    # for the odd ones: the name decides the ORDER, the content the FORMAT
    (d / "x.csi").write_bytes(csi)
    assert fmt() == "csi"
    (d / "x.bam.csi").write_bytes(bai)
    assert fmt() == "bai"
    (d / "x.bai").write_bytes(csi)
    assert fmt() == "csi"
    (d / "x.bam.bai").write_bytes(bai)
    assert fmt() == "bai"
    assert sorted(os.listdir(d)) == sorted(names + ["x.bam"])
    with bam.BamFile(bam_path, index=False) as bf:
        assert bf.index_format is None and not bf.has_index


# ------------------------------------------------------------------------------------------------ under the sanitizers
def test_the_parser_and_bytes_csi_under_the_sanitizers_equal_the_library(big, small, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (the library's own build needs it too)"
    exe, corpus = str(tmp_path / "csi_core_main"), str(tmp_path / "corpus.bin")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "csi_core_main.cpp")], check=True, capture_output=True, text=True)
    path, _, info, _ = big
    p = info["payload"]
    payloads = [p, p[:-8], cw.write_csi(path, str(tmp_path / "a.csi"), 12, 6)["payload"], cw.write_csi(path, str(tmp_path / "b.csi"), pseudo=False)["payload"],
                b"CSJ\1" + p[4:], _put(p, 4, "<i", 0), _put(p, cw.fields(p)["n_bin_at"][1], "<i", 1 << 30), b"", b"CSI\1"]
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(payloads)))
        for q in payloads:
            f.write(struct.pack("<I", len(q)) + q)
    r = subprocess.run([exe, corpus, "2"], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1].startswith("ok ") and int(lines[-1].split()[1]) > 10000, (r.stdout[-2000:], r.stderr[-2000:])
    for i, q in enumerate(payloads):
        got = lines[i].split()
        with bam.BamFile(path, index=False) as bf:
            try:
                bf.load_index(cw.write_payload(tmp_path / "q.csi", q))
            except bam.BamError:
                assert got[1] == "0", (i, got)
                continue
            st = bf.index_statistics()
            assert got[1] == "1" and int(got[5]) == sum(s[1] for s in st) and int(got[6]) == sum(s[2] for s in st), (i, got)
            assert int(got[7]) == (-1 if bf.no_coordinate is None else bf.no_coordinate)
            for k, pos in ((8, 0), (9, 1 << 29)):
                assert bf.index_block("huge", pos) == _block_of(info, int(got[k])), (i, got)
