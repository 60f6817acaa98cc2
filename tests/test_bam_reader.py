"""The native BAM reader (cutesv_amd/bam.py, csrc/bam_host.cpp, csrc/bam.hip.h): files written by tests/bam_writer.py - an
independent reading of the SAM/BAM specification - read back and compared, column for column and without tolerances, with
what tests/helpers.py:StubRecord reports for the same record; `extract.single_pipe_bam` against the reference's recorded
single_pipe output.  CPU tests use `bam.decode_host`; the GPU tests (-m gpu) compare `bam.decode` with it and run the
device path end to end.

Every record of parse_reads.json.gz and single_pipe.json.gz can be written as BAM (test_every_golden_record_is_representable
checks the field ranges); none of them has an empty CIGAR (it would become n_cigar_op = 0; test_edge_records has one)."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from cutesv_amd import bam, extract, synth, _abi, _lib
from helpers import load_json, StubRecord
import bai_writer
import bam_writer
import frame_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = {"1": 248956422, "10": 133797422, "2": 242193529, "7": 159345973, "X": 156040895}
PER_RECORD = ("ref_start", "ref_end", "flag", "mapq", "query_len", "clip_left", "clip_right", "cls", "status", "cg_beg", "cg_end")


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def golden_records(case, chrom):
    """the records of a parse_reads / single_pipe case as the writer takes them (+ the refs of the header)"""
    refs = [(c, REF_LEN[c]) for c in case["chroms"]]
    refid = case["chroms"].index(chrom)
    recs = [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=refid, tags=[tuple(t) for t in d["tags"]]) for d in case["reads"]]
    return refs, recs


def all_cases():
    return ([("parse_reads", c, c["chrom"]) for c in load_json("parse_reads.json.gz")] +
            [("single_pipe", c, c["task"][0]) for c in load_json("single_pipe.json.gz")])


def read_all(path, chrom, **kw):
    """every chunk of a contig, decoded on the host -> [(chunk, columns)]"""
    with bam.BamFile(path, threads=2) as bf:
        return [(ch, bam.decode_host(ch)) for ch in bf.chunks(chrom, **kw)]


def assert_matches_stubs(parts, dicts):
    """the decoded chunks `parts` hold exactly the records `dicts`, in order: every column, names, sequences, CIGARs, SA values"""
    stubs = [StubRecord(d) for d in dicts]
    assert sum(ch.n for ch, _ in parts) == len(stubs)
    k = 0
    for ch, cols in parts:
        mine = stubs[k : k + ch.n]
        k += ch.n
        assert cols["ref_start"].tolist() == [s.reference_start for s in mine]
        assert cols["ref_end"].tolist() == [s.reference_end for s in mine]
        assert cols["flag"].tolist() == [s.flag for s in mine]
        assert cols["mapq"].tolist() == [s.mapq for s in mine]
        assert cols["query_len"].tolist() == [s.query_length for s in mine]
        assert cols["cls"].tolist() == [0 if s.flag in (256, 272) else 1 if s.flag in (0, 16) else 2 for s in mine]
        ct = [s.cigartuples or [(0, 0)] for s in mine]
        assert cols["clip_left"].tolist() == [c[0][1] if c[0][0] in (4, 5) else 0 for c in ct]
        assert cols["clip_right"].tolist() == [c[-1][1] if c[-1][0] in (4, 5) else 0 for c in ct]
        assert not cols["status"].any()
        off, flat = extract.encode_cigars([s.cigartuples for s in mine])
        assert np.array_equal(cols["cig_off"], off) and np.array_equal(cols["cigar"], flat)
        assert cols["cigar"].dtype == np.uint32 and cols["cig_off"].dtype == np.int64
        for i, s in enumerate(mine):
            assert ch.name(i) == s.query_name
            assert ch.sequence(i) == s.query_sequence
            assert ch.sa_values(cols, i) == [t[-1] for t in s.get_tags() if t[0] == "SA"]


def assert_columns_equal(a, b, where=""):
    for k in bam.COLUMNS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (where, k)


# ------------------------------------------------------------------------------------------------ CPU
def test_every_golden_record_is_representable():
    """BAM's field widths hold every golden record: nothing has to be dropped or altered on the way into a file"""
    n = 0
    for _, case, chrom in all_cases():
        for d in case["reads"]:
            assert 0 <= d["flag"] < 65536 and 0 <= d["mapq"] < 256 and 0 <= d["start"] < 2 ** 31 and 0 < len(d["name"]) < 255
            assert all(0 <= op <= 9 and 0 <= ln < 2 ** 28 for op, ln in d["cigar"]) and d["seq_len"] < 2 ** 28
            assert all((isinstance(v, int) and -2 ** 31 <= v < 2 ** 31) or isinstance(v, str) for _, v in d["tags"])
            assert set(synth.pseudo_sequence(min(d["seq_len"], 64), d["seq_key"])) <= set("=ACMGRSVTWYHKDBN")
            n += 1
    assert n == 1900


@pytest.mark.parametrize("which", range(5))
def test_golden_records_round_trip(tmp_path, which):
    kind, case, chrom = all_cases()[which]
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "a.bam")
    bam_writer.write_bam(path, refs, recs)
    with bam.BamFile(path) as bf:
        assert bf.references == [r for r, _ in refs] and bf.lengths == [ln for _, ln in refs] and bf.sort_order == "coordinate"
        for other in bf.references:
            assert bf.count(other) == (len(recs) if other == chrom else 0)
    assert_matches_stubs(read_all(path, chrom), case["reads"])
    assert_matches_stubs(read_all(path, chrom, chunk_records=37), case["reads"])            # many chunks


def _single_pipe_bam_case(case, path, fns):
    """The fixture was recorded with a stub alignment file whose fetch() ignores the region and yields EVERY record of the
    case (tests/golden/make_golden_parse.py: the reference's single_pipe uses the task's end nowhere else), and in the case
    "plain" a third of the records start behind the task's end.  A real fetch does not yield those, and neither does
    BamFile.records.  So that the reader presents the alignments the recorded run saw, the region's end is moved behind the
    last record here; the task's start - the gate the reference applies itself - is the case's.  The case's own end is
    covered by test_single_pipe_bam_region_equals_the_object_path."""
    p = case["params"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    chrom, t0, t1 = case["task"]
    t1 = max(t1, max(d["start"] for d in case["reads"]) + 1)
    with bam.BamFile(path) as bf:
        cand, reads_info = extract.single_pipe_bam(fns, bf, chrom, t0, t1, rank, p["sv"], p["min_mapq"], p["parts"], p["min_read_len"], p["min_siglength"],
                                                   p["md"], p["mi"], p["max_size"], bed_regions=case["bed"])
    for t in ("DEL", "INS", "DUP", "INV", "TRA"):                      # (the comparison of helpers.assert_single_pipe_case)
        got = [list(x) for x in cand[t]]
        assert got == case[t], (case["name"], t, len(got), len(case[t]))
    assert [list(x) for x in reads_info] == case["reads_table"], (case["name"], len(reads_info), len(case["reads_table"]))
    assert len(reads_info) > 20


def test_single_pipe_bam_equals_the_reference(tmp_path):
    """the acceptance check: single_pipe_bam with the oracle's functions and decode_host == the reference's recorded single_pipe"""
    o = _oracle()
    cases = load_json("single_pipe.json.gz")
    assert len(cases) == 2
    for case in cases:
        refs, recs = golden_records(case, case["task"][0])
        path = str(tmp_path / (case["name"] + ".bam"))
        bam_writer.write_bam(path, refs, recs)
        _single_pipe_bam_case(case, path, (o.cigar_signatures, o.split_signatures))


def _region_case(case, path, fns, object_fns):
    """single_pipe_bam on the case's own region == single_pipe on the StubRecords a fetch of that region yields"""
    p = case["params"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    chrom, t0, t1 = case["task"]
    args = (p["sv"], p["min_mapq"], p["parts"], p["min_read_len"], p["min_siglength"], p["md"], p["mi"], p["max_size"])
    stubs = [s for s in (StubRecord(d) for d in case["reads"]) if s.reference_start < t1 and max(s.reference_end, s.reference_start + 1) > t0]
    assert 20 < len(stubs) < len(case["reads"])
    want = extract.single_pipe(stubs, chrom, t0, rank, *args, *object_fns, bed_regions=case["bed"])
    with bam.BamFile(path) as bf:
        got = extract.single_pipe_bam(fns, bf, chrom, t0, t1, rank, *args, bed_regions=case["bed"])
    assert got == want
    assert sum(len(v) for v in got[0].values()) > 50 and len(got[1]) > 10


def test_single_pipe_bam_region_equals_the_object_path(tmp_path):
    o = _oracle()
    for case in load_json("single_pipe.json.gz"):
        refs, recs = golden_records(case, case["task"][0])
        path = str(tmp_path / (case["name"] + ".bam"))
        bam_writer.write_bam(path, refs, recs)
        _region_case(case, path, (o.cigar_signatures, o.split_signatures), (o.cigar_signatures, o.split_signatures))


def test_parse_reads_results_unchanged():
    """the factoring of parse_reads (shared with single_pipe_bam) keeps its results: the golden cases through the oracle"""
    from helpers import assert_parse_case
    o = _oracle()
    for case in load_json("parse_reads.json.gz"):
        assert_parse_case(case, o.cigar_signatures, o.split_signatures)


def test_framing_is_independent_of_block_cuts(tmp_path):
    case = load_json("single_pipe.json.gz")[0]
    refs, recs = golden_records(case, "7")
    base = str(tmp_path / "base.bam")
    info = bam_writer.write_bam(base, refs, recs)                       # 64 KB blocks: records span them freely
    assert info["n_blocks"] > 10
    want = read_all(base, "7")
    assert_matches_stubs(want, case["reads"])
    r5, r9, r11 = info["records"][5], info["records"][9], info["records"][11]
    variants = {"record": "record",
                "inside": [r5["offset"] + 2, r5["fixed"] + 13, r9["cigar"] + 6, r11["aux"] + 5, r11["aux"] + 6, info["header_end"] - 3, 9],
                "small": list(range(1000, info["records"][-1]["end"], 1777))}
    for name, cuts in variants.items():
        path = str(tmp_path / (name + ".bam"))
        bam_writer.write_bam(path, refs, recs, cuts=cuts)
        got = read_all(path, "7")
        assert len(got) == len(want) == 1
        assert_columns_equal(got[0][1], want[0][1], name)
        assert np.array_equal(got[0][0].slim, want[0][0].slim) and np.array_equal(got[0][0].host, want[0][0].host)


def edge_records():
    """records that exercise the CG tag, every tag type around SA, empty CIGARs and the CIGAR-pass tiers (0, 1, 63, 64, 65,
    4 096 and 70 000 operations in one chunk)"""
    rng = np.random.RandomState(7)
    every = [("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 250), ("Xs", "s", -30000), ("XS", "S", 65000), ("Xi", "i", -2 ** 31), ("XI", "I", 2 ** 32 - 1),
             ("Xf", "f", 1.5), ("XZ", "Z", "text SA:Z:decoy"), ("XH", "H", "1AE301"), ("B0", "B", ("c", [-1, 2, 3])), ("B1", "B", ("C", [1, 2, 255])),
             ("B2", "B", ("s", [-7, 7])), ("B3", "B", ("S", [65535])), ("B4", "B", ("i", [-9, 9, 10])), ("B5", "B", ("I", [4000000000])),
             ("B6", "B", ("f", [0.25, -1.0])), ("B7", "B", ("C", []))]
    sa1, sa2 = "1,2239803,-,2063S670M3490S,0,3;", "7,1126818,+,4783S1899M,60,3;X,5,-,10S20M,1,0;"
    recs, pos = [], 1000

    def add(n_ops, tags, flag=0, cg=False, name=None):
        nonlocal pos
        ops = []
        for k in range(n_ops):                              # clips at the ends, then M / I / D / = / X / N in turn
            op = 4 if k == 0 and n_ops > 1 else 5 if k == n_ops - 1 and n_ops > 2 else (0, 1, 0, 2, 7, 8, 3)[k % 7]
            ops.append((op, int(rng.randint(1, 40))))
        qlen = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        recs.append(dict(name=name or "e%05d" % len(recs), flag=flag, mapq=int(rng.randint(0, 61)), start=pos, cigar=ops, seq_len=qlen,
                         seq_key=1000 + len(recs), tags=tags, cg=cg))
        pos += int(rng.randint(0, 500))

    add(0, [("NM", 3)])
    add(1, [("SA", sa1)] + every)
    add(63, every + [("SA", sa1)], flag=16)
    add(64, every[:9] + [("SA", sa1)] + every[9:] + [("SA", sa2)])
    add(65, [], flag=2048)
    add(4096, [("NM", 1)], flag=256)
    add(70000, [("Xc", "c", 1), ("SA", sa2)], flag=16)                    # CG because it must
    add(5000, every[10:13] + [("SA", sa1)], cg=True)                    # CG by choice, behind tags of odd total length
    add(12, [("XA", "A", "x")], cg=True, flag=272, name="q" * 254)       # the longest name a record can hold
    add(3, [("CG", "B", ("I", [5 << 4]))])                              # a CG tag without the placeholder: the record's own CIGAR counts
    return recs


def write_edge(path, cg_rows=True, **kw):
    recs = edge_records()
    out = [dict(r, seq=synth.pseudo_sequence(r["seq_len"], r["seq_key"]), refid=0) for r in recs]
    # the writer's cg switch is per file: records that ask for it are pre-encoded one by one through record_bytes in info order
    info = _write_mixed(path, [("7", REF_LEN["7"]), ("X", REF_LEN["X"])], out, **kw)
    return recs, info


def _write_mixed(path, refs, recs, **kw):
    """write_bam with the CG form chosen per record (the dict's `cg`)"""
    orig = bam_writer.record_bytes
    try:
        bam_writer.record_bytes = lambda r, cg=False: orig(r, cg=bool(r.get("cg")))
        return bam_writer.write_bam(path, refs, recs, **kw)
    finally:
        bam_writer.record_bytes = orig


def test_edge_records(tmp_path):
    path = str(tmp_path / "edge.bam")
    recs, info = write_edge(path)
    parts = read_all(path, "7")
    assert_matches_stubs(parts, recs)
    ch, cols = parts[0]
    n_ops = np.diff(cols["cig_off"]).tolist()
    assert n_ops == [0, 1, 63, 64, 65, 4096, 70000, 5000, 12, 3]
    assert (cols["cg_beg"] >= 0).tolist() == [False] * 6 + [True] * 4
    assert ((cols["cg_end"] - cols["cg_beg"]) // 4).tolist()[6:] == [70000, 5000, 12, 1]
    assert np.diff(cols["sa_off"]).tolist() == [0, 1, 1, 2, 0, 0, 1, 1, 0, 0]
    assert ch.stats["upload_bytes_per_record"] < ch.stats["inflated_bytes_per_record"]          # sequences and qualities stay behind
    # cut inside the 70 000-operation CG array and its neighbours: the same columns
    r6 = info["records"][6]
    path2 = str(tmp_path / "edge_cut.bam")
    write_edge(path2, cuts=[r6["aux"] + 11, r6["aux"] + 100001, r6["end"] - 1, r6["offset"] + 3])
    assert_columns_equal(read_all(path2, "7")[0][1], cols)


def test_two_contigs_and_unmapped_tail(tmp_path):
    case = load_json("single_pipe.json.gz")[1]
    refs, recs = golden_records(case, "7")
    a = [dict(r, refid=1) for r in recs[:100]]              # contig "10"
    b = [dict(r, refid=3) for r in recs[100:]]              # contig "7"
    tail = [dict(recs[k], refid=-1, start=-1, cigar=[], flag=4, mapq=0, tags=[]) for k in range(7)]
    path = str(tmp_path / "two.bam")
    bam_writer.write_bam(path, refs, a + b + tail, block_bytes=20000)
    with bam.BamFile(path, threads=3) as bf:
        assert [bf.count(c) for c in bf.references + [None]] == [0, 100, 0, 200, 0, 7]
        # any order of access: contigs are found by scanning forward and remembered
        assert_matches_stubs([(ch, bam.decode_host(ch)) for ch in bf.chunks("7", chunk_records=64)], case["reads"][100:])
        assert_matches_stubs([(ch, bam.decode_host(ch)) for ch in bf.chunks("10")], case["reads"][:100])
        assert list(bf.chunks("2")) == [] and list(bf.chunks("X")) == []
        (ch,) = list(bf.chunks(None))
        cols = bam.decode_host(ch)
        assert ch.n == 7 and cols["ref_start"].tolist() == [-1] * 7 and cols["cig_off"].tolist() == [0] * 8 and cols["cls"].tolist() == [2] * 7
        assert [ch.name(i) for i in range(7)] == [r["name"] for r in recs[:7]]
        # regions: what an overlap test on every record selects
        stubs = [StubRecord(d) for d in case["reads"][100:]]
        for lo, hi in ((0, 1), (700000, 900000), (1500000, 1500001), (2987850, 2987851), (2999999, 10 ** 9), (600000, 600000 + 5), (0, 10 ** 9)):
            want = [s.query_name for s in stubs if s.reference_start < hi and max(s.reference_end, s.reference_start + 1) > lo]
            got = bf.records("7", lo, hi)
            assert [got.name(i) for i in range(got.n)] == want, (lo, hi)
        with pytest.raises(KeyError):
            bf.records("nope", 0, 10)


def test_broken_files_raise(tmp_path):
    case = load_json("single_pipe.json.gz")[0]
    refs, recs = golden_records(case, "7")
    p = lambda n: str(tmp_path / n)                                                # noqa: E731
    bam_writer.write_bam(p("unsorted.bam"), refs, recs, sort_order="unsorted")
    with pytest.raises(bam.BamError, match="SO:unsorted"):
        bam.BamFile(p("unsorted.bam"))
    bam_writer.write_bam(p("noeof.bam"), refs, recs, eof=False)
    with pytest.raises(bam.BamError, match="end-of-file block"):
        bam.BamFile(p("noeof.bam"))
    bam_writer.write_bam(p("trunc.bam"), refs, recs, eof=False, truncate=1000)     # the last data block is cut short
    with pytest.raises(bam.BamError, match="truncated"):
        bam.BamFile(p("trunc.bam"))
    bam_writer.write_bam(p("trunc2.bam"), refs, recs, truncate=5)                  # the EOF block itself is cut
    with pytest.raises(bam.BamError, match="truncated"):
        bam.BamFile(p("trunc2.bam"))
    # a stream that ends inside a record (whole blocks, EOF block present)
    info = bam_writer.write_bam(p("full.bam"), refs, recs, cuts="record")
    blob = open(p("full.bam"), "rb").read()
    last = bam_writer.bgzf_block(b"\x40\x00\x00\x00" + b"\0" * 20)
    open(p("short.bam"), "wb").write(blob[:-28] + last + bam_writer.EOF_BLOCK)
    with bam.BamFile(p("short.bam")) as bf:
        with pytest.raises(bam.BamError, match="ends inside a record"):
            list(bf.chunks("7"))
    # a damaged payload fails its CRC
    bad = bytearray(blob)
    bad[len(blob) // 2] ^= 0x55
    open(p("crc.bam"), "wb").write(bytes(bad))
    with pytest.raises(bam.BamError):
        with bam.BamFile(p("crc.bam")) as bf:
            list(bf.chunks("7"))
    open(p("text.bam"), "wb").write(b"not a bam file at all, but long enough to be looked at")
    with pytest.raises(bam.BamError):
        bam.BamFile(p("text.bam"))
    with pytest.raises(bam.BamError):
        bam.BamFile(p("missing.bam"))


def malformed_chunk(tmp_path):
    """a chunk whose record 1 has an unknown tag type and whose record 3 has a Z value without its NUL"""
    path = str(tmp_path / "ok.bam")
    recs = [dict(name="m%d" % i, flag=0, mapq=30, start=100 + i, cigar=[(0, 50)], seq="A" * 50, tags=[("NM", 1), ("XZ", "Z", "hello")]) for i in range(5)]
    bam_writer.write_bam(path, [("7", 1000)], recs)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    o1, o3 = int(ch.rec_off[1]), int(ch.rec_off[3])
    ch.slim[o1 + 32 + 4 + 2] = ord("?")                     # the type byte of NM
    ch.slim[o3 + int(ch.rec_len[3]) - 1] = ord("!")         # the NUL that ends XZ, the record's last byte
    return ch


def test_malformed_tags_set_status_and_raise(tmp_path):
    ch = malformed_chunk(tmp_path)
    with pytest.raises(bam.BamError, match="malformed"):
        bam.decode_host(ch)
    cols = bam.decode_host(ch, check=False)
    assert cols["status"].tolist() == [0, 1, 0, 1, 0]
    assert cols["ref_start"].tolist() == [100, 101, 102, 103, 104] and np.diff(cols["cig_off"]).tolist() == [1] * 5


def test_abi_has_the_bam_entries():
    L = _lib.lib()
    assert _abi.ABI_VERSION == 9 and L.csv_abi_version() == 9
    assert [L.csv_bam_struct_size(i) for i in range(4)] == [C.sizeof(bam.ChunkC), C.sizeof(bam.BamIn), C.sizeof(bam.BamOut), -1]
    assert hasattr(L, "csv_bam_decode") and _abi.CG_FROM_BAM == 2
    assert 1 <= bam.default_threads() <= 16


def test_command_line(tmp_path):
    path = str(tmp_path / "edge.bam")
    recs, _ = write_edge(path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "cutesv_amd.bam", path, "--chrom", "7", "--dump-columns", str(tmp_path / "cols")],
                         cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert "@HD\tVN:1.6\tSO:coordinate" in out and "@SQ\tSN:X" in out and "\n7\t%d\n" % len(recs) in out
    assert np.load(str(tmp_path / "cols" / "ref_start.npy")).tolist() == [r["start"] for r in recs]
    assert np.load(str(tmp_path / "cols" / "cig_off.npy"))[-1] == sum(len(r["cigar"]) for r in recs)
    out = subprocess.run([sys.executable, "-m", "cutesv_amd.bam", path], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.endswith("7\t%d\nX\t0\n*\t0\n" % len(recs))


def _host_main_expected(path, ops):
    """the lines tests/bam_host_main.cpp prints for `ops` on `path`, from BamFile of the product library"""
    crc = lambda a: zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF       # noqa: E731
    own = lambda e: str(e)[len(path) + 2:] if str(e).startswith(path + ": ") else str(e)      # noqa: E731  (BamFile puts the path in front)
    try:
        bf = bam.BamFile(path, threads=2, index=False)
    except bam.BamError as e:
        return ["open: " + own(e)]
    lines = []
    with bf:
        for op in ops:
            name, _, rest = op.partition(":")
            f = rest.split(":")
            chrom = None if not rest or int(f[0]) < 0 else bf.references[int(f[0])]
            try:
                if name == "load":
                    lines.append("load ok" if bf.load_index(required=False) else "load none")
                elif name == "drop":
                    bf.drop_index()
                elif name == "build":
                    st = bf.build_index()
                    lines.append("build bytes=%d crc=%08x records=%d" % (st["index_bytes"], crc(np.frombuffer(bf.index_bytes(), np.uint8)), st["records"]))
                elif name == "count":
                    lines.append("count %d" % bf.count(chrom))
                else:
                    beg, end, k, ranges = {"chunks": lambda: (-bam.ALL, bam.ALL, int(f[1]), None), "region": lambda: (int(f[1]), int(f[2]), (1 << 31) - 8192, None),
                                           "ranges": lambda: (-bam.ALL, bam.ALL, int(f[1]), bf._ranges([int(x) for x in f[2].split(",")]))}[name]()
                    flags = _abi.BAM_RESTART
                    while True:
                        ch = bf._read(chrom, beg, end, k, flags, ranges)
                        lines.append("chunk n=%d more=%d slim=%d:%08x rec_off=%08x rec_len=%08x host=%d:%08x host_off=%08x"
                                     % (ch.n, ch.more, len(ch.slim), crc(ch.slim), crc(ch.rec_off), crc(ch.rec_len), len(ch.host), crc(ch.host), crc(ch.host_off)))
                        if not ch.more:
                            break
                        flags = 0
            except bam.BamError as e:
                lines.append(("load error: " if name == "load" else "error: ") + own(e))
    return lines


def test_host_route_under_the_sanitizers(tmp_path):
    """bam_host.cpp in a stand-alone program (tests/bam_host_main.cpp) built with -fsanitize=address,undefined: the window refills with
    their kept tail, the packing of both images, index load and build, and the damaged files.  The program exits cleanly - no
    sanitizer report - and every line it prints is what BamFile of the product library says of the same read on the same file."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed to build tests/bam_host_main.cpp")
    exe = str(tmp_path / "bam_host_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "bam_host_main.cpp"), os.path.join(ROOT, "cutesv_amd", "csrc", "bam_host.cpp"), "-lz", "-pthread"],
                   check=True, capture_output=True, text=True)
    p = lambda n: str(tmp_path / n)                                                # noqa: E731
    _, case, chrom = all_cases()[0]
    refs, recs = golden_records(case, chrom)
    recs.sort(key=lambda d: d["start"])                                            # (the case lists its reads in no order; an index needs a sorted file)
    refid = case["chroms"].index(chrom)
    starts = [d["start"] for d in recs]
    lo, mid, hi = starts[len(starts) // 3], starts[len(starts) // 2], starts[2 * len(starts) // 3]
    reads = ["chunks:%d:37" % refid, "region:%d:%d:%d" % (refid, lo, hi), "ranges:%d:50:%d,%d,%d,%d,%d,%d" % (refid, starts[3], starts[9] + 1, lo, lo + 1, mid, hi),
             "count:%d" % refid, "count:-1", "region:%d:%d:%d" % (refid, starts[-1] + 10 ** 7, starts[-1] + 10 ** 7 + 1)]
    files = []
    for name, kw in (("default", {}), ("small", dict(block_bytes=512))):
        for with_bai in (False, True):
            path = p("%s%d.bam" % (name, with_bai))
            info = bam_writer.write_bam(path, refs, recs, **kw)
            if with_bai:
                bai_writer.write_bai(path)
            # without a .bai: the forward scan, then a build and the same reads through the built index; with one: the loaded index,
            # then the forward scan again
            files.append((path, ["load"] + reads + (["drop"] + reads[:3] if with_bai else ["build"] + reads)))
        assert name == "default" or info["n_blocks"] > 8 * 256                     # the 256-block window is refilled many times, records crossing its edges
    # the damaged files: a truncated file, a stream that ends inside a record and inside a block_size word, block_size < 32, fields
    # that exceed block_size
    short = frame_helpers.short_records(400)
    info = bam_writer.write_bam(p("full.bam"), frame_helpers.REFS, short, cuts="record")
    blob = open(p("full.bam"), "rb").read()
    bam_writer.write_bam(p("trunc.bam"), refs, recs, eof=False, truncate=1000)
    tails = {"small.bam": struct.pack("<i", 31) + b"\0" * 40, "short.bam": b"\x40\x00\x00\x00" + b"\0" * 20, "short2.bam": b"\x40\x00"}
    for name, tail in tails.items():
        open(p(name), "wb").write(blob[:-28] + bam_writer.bgzf_block(tail) + bam_writer.EOF_BLOCK)
    stream, lens = frame_helpers.stream_of(p("full.bam"))
    bad = bytearray(stream)
    struct.pack_into("<I", bad, info["records"][200]["fixed"] + 16, 1 << 20)        # l_seq of record 200 says more than the record holds
    cuts = np.r_[0, np.cumsum(lens[:-1])]
    open(p("fields.bam"), "wb").write(b"".join(bam_writer.bgzf_block(bytes(bad[a:b])) for a, b in zip(cuts[:-1], cuts[1:])) + bam_writer.EOF_BLOCK)
    files += [(p(n), ["chunks:0:50", "count:0", "build"]) for n in ("trunc.bam", "small.bam", "short.bam", "short2.bam", "fields.bam")]
    seen = set()
    for path, ops in files:
        run = subprocess.run([exe, path, "2"] + ops, capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", (path, run.returncode, run.stderr[-2000:])
        got, want = run.stdout.splitlines(), _host_main_expected(path, ops)
        assert got == want, (path, [(g, w) for g, w in zip(got, want) if g != w][:3], len(got), len(want))
        if ops[0] == "load":                                                        # the sound files: the index is loaded or built, and every read has records
            assert got[0] == ("load ok" if "drop" in ops else "load none") and ("drop" in ops or any(ln.startswith("build bytes=") for ln in got))
            assert not any(ln.startswith("error") for ln in got) and sum(ln.startswith("chunk n=") and " n=0 " not in ln for ln in got) > 2 * 400 // 37
        seen.update(ln.split(" at ")[0].split(" byte ")[0] for ln in got if ln.startswith(("error", "open")))
    assert len(seen) >= 4, seen                                                     # the damaged files fail in their different ways


# ------------------------------------------------------------------------------------------------ GPU
def _device_equals_host(ctx, chunk, where=""):
    want = bam.decode_host(chunk)
    got = bam.decode(ctx, chunk)
    assert_columns_equal(got, want, where)
    assert got["n_ops"] == want["n_ops"] and got["n_sa"] == want["n_sa"] and (got["ms_device"] > 0 or chunk.n == 0)
    assert got["bytes_uploaded"] == len(chunk.slim) + 12 * chunk.n
    return got


@pytest.mark.gpu
def test_gpu_decode_equals_host_on_the_goldens(ctx, tmp_path):
    for kind, case, chrom in all_cases():
        refs, recs = golden_records(case, chrom)
        path = str(tmp_path / "g.bam")
        bam_writer.write_bam(path, refs, recs)
        with bam.BamFile(path) as bf:
            for kw in ({}, {"chunk_records": 37}):
                for ch in bf.chunks(chrom, **kw):
                    _device_equals_host(ctx, ch, case["name"])


@pytest.mark.gpu
def test_gpu_decode_edge_records_and_every_cigar_tier(ctx, tmp_path):
    path = str(tmp_path / "edge.bam")
    recs, _ = write_edge(path)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    got = _device_equals_host(ctx, ch)
    assert np.diff(got["cig_off"]).tolist() == [0, 1, 63, 64, 65, 4096, 70000, 5000, 12, 3]
    assert_matches_stubs([(ch, got)], recs)
    # the unmapped tail and an empty region
    case = load_json("single_pipe.json.gz")[1]
    refs, g = golden_records(case, "7")
    tail = [dict(g[k], refid=-1, start=-1, cigar=[], flag=4, mapq=0, tags=[]) for k in range(7)]
    path = str(tmp_path / "tail.bam")
    bam_writer.write_bam(path, refs, g[:50] + tail)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks(None))
        _device_equals_host(ctx, ch)
        empty = bf.records("7", 10 ** 9, 10 ** 9 + 1)
        assert empty.n == 0
        _device_equals_host(ctx, empty)


@pytest.mark.gpu
def test_gpu_malformed_tag_fails_with_invalid(ctx, tmp_path):
    from cutesv_amd.engine import CsvError
    ch = malformed_chunk(tmp_path)
    with pytest.raises(CsvError) as e:
        bam.decode(ctx, ch)
    assert e.value.code == _abi.E_INVALID
    # ... and a chunk whose offsets leave the image is refused before any kernel runs
    ch2 = malformed_chunk(tmp_path)
    ch2.rec_len[4] += 64
    with pytest.raises(CsvError) as e:
        bam.decode(ctx, ch2)
    assert e.value.code == _abi.E_INVALID


@pytest.mark.gpu
def test_gpu_single_pipe_bam_equals_the_reference(ctx, tmp_path):
    for case in load_json("single_pipe.json.gz"):
        refs, recs = golden_records(case, case["task"][0])
        path = str(tmp_path / (case["name"] + ".bam"))
        bam_writer.write_bam(path, refs, recs)
        _single_pipe_bam_case(case, path, ctx)
        o = _oracle()
        _region_case(case, path, ctx, (o.cigar_signatures, o.split_signatures))


@pytest.mark.gpu
def test_gpu_cigar_scan_from_device_columns(ctx, tmp_path):
    """CSV_CG_FROM_BAM: the scan on the columns the decode left on the device == the scan on the same columns uploaded"""
    path = str(tmp_path / "edge.bam")
    write_edge(path)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    cols = bam.decode(ctx, ch)
    use = np.ones(ch.n, np.uint8)
    a = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
    b = extract.cigar_signatures(ctx, cols["cig_off"], cols["cigar"], cols["ref_start"], use, min_siglength=5)
    want = _oracle().cigar_signatures(cols["cig_off"], cols["cigar"], cols["ref_start"], use, min_siglength=5)
    for k in ("ins_read", "ins_pos", "ins_len", "ins_piece0", "ins_npiece", "piece_qoff", "piece_len", "del_read", "del_pos", "del_len"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], want[k]), k
    assert a["n_sig_ins"] > 100 and a["n_sig_del"] > 100
    from cutesv_amd.engine import CsvError
    with pytest.raises(CsvError):                           # the record count must be the decode's
        extract.cigar_signatures(ctx, None, None, None, use[:-1], from_bam=dict(cols, ref_start=cols["ref_start"][:-1]))


@pytest.mark.gpu
def test_gpu_export_and_struct_sizes(ctx):
    test_abi_has_the_bam_entries()
