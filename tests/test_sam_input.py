"""SAM text -> BAM: cutesv_amd.sam, csv_sam_to_bam / csv_sam_to_bam_host / csv_sam_records, sam_core.h.

The judge is tests/sam_helpers.py: an independent SAM line writer and an independent line -> record function from the specification
(float(text) packed "<f"), which import nothing of the package.  Equality is on the inflated stream byte for byte; between the host and
the device route on the file byte for byte.  CPU: the core under the sanitizers (tests/sam_core_main.cpp), the host route on every
crafted case, every refusal by its line, the header cases, window independence, files and command lines.  GPU: the device route on
cases aimed at its seams - tile edges of the mark pass, 16-byte store edges of the bulk pass, block edges, windows - against the
judge's stream and the host route's file.  `cli.main --sort_input host` on SAM text runs under the gpu mark too: the calling itself needs
the device whatever the sort's route."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_writer
import call_helpers
import sam_helpers as sh
import sort_helpers
from cutesv_amd import bam, cli, sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS2 = [("c1", 100000), ("c2", 80000)]
BIG = (1 << 31) - 1
TILE, WAVE_BYTES, STEP = 32768, 8192, 1024                 # the mark pass: a workgroup's tile, a wavefront's share, a wavefront's step


# ------------------------------------------------------------------------------------------------ the cases
def _seq(n, seed=0):
    rng = np.random.default_rng(seed + 1000 * n)
    return "".join(rng.choice(list("ACGT"), n)) if n else ""


def _qual(n, seed=0):
    rng = np.random.default_rng(seed + 7 + 1000 * n)
    return "".join(chr(int(c)) for c in rng.integers(33, 127, n)) if n else "*"


def _plain(n, seed=1, qual=True):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(0, 60))
        out.append(sh.tiny("r%d" % i, int(rng.integers(0, 2)), int(rng.integers(0, 70000)), flag=int(rng.choice([0, 16, 256, 2048])), seq=_seq(ln, i),
                           qual=_qual(ln, i) if qual and i % 3 else "*", tags=[("NM", int(rng.integers(0, 500))), ("de", "f", "0.%04d" % int(rng.integers(0, 9999)))][: i % 3]))
    return out


def _int_borders():
    vals = set()
    for b in (-(1 << 31), -32768, -128, -1, 0, 255, 65535, (1 << 32) - 1):
        vals.update(v for v in (b - 1, b, b + 1) if -(1 << 31) <= v <= (1 << 32) - 1)
    return sorted(vals)


FAST_FLOATS = ["0", "-0.0", "1", "0.1", "3.14159", "123456789012345", "1e22", "1e-22", "9.5e-8", "0.000001", "16777217", "0.0123", "1E5", "+2.5e+3", "0.0517"]
SLOW_FLOATS = ["1234567890123456", "1e23", "1e-40", "0.1234567890123456", "1e-23"]
HOST_FLOATS = ["inf", "nan", "-inf", "1.", ".5"]              # outside the grammar: strtod on the host, counted as patches too


def _tags_case():
    recs = []
    for i, v in enumerate(_int_borders()):
        recs.append(sh.tiny("i%d" % i, 0, 10 + i, tags=[("XI", "i", v)]))
    for i, t in enumerate(FAST_FLOATS + SLOW_FLOATS + HOST_FLOATS):
        recs.append(sh.tiny("f%d" % i, 1, 10 + i, tags=[("de", "f", t), ("NM", 3)]))
    subs = dict(c=[-128, 127, -1], C=[0, 255, 7], s=[-32768, 32767, 5], S=[0, 65535, 9], i=[-(1 << 31), BIG, 0], I=[0, (1 << 32) - 1, 1])
    for sub, vals in subs.items():
        for n in (0, 1, 65):
            recs.append(sh.tiny("b%s%d" % (sub, n), 0, 500 + n, tags=[("XB", "B", (sub, [vals[k % 3] for k in range(n)])), ("XA", "A", "q")]))
    for n in (0, 1, 65):
        recs.append(sh.tiny("bf%d" % n, 0, 600 + n, tags=[("XF", "B", ("f", (FAST_FLOATS + SLOW_FLOATS)[:n] if n < 65 else (FAST_FLOATS + SLOW_FLOATS + FAST_FLOATS * 4)[:65]))]))
    recs.append(sh.tiny("hz", 0, 700, tags=[("XH", "H", "1AE301ff"), ("XE", "H", ""), ("XZ", "Z", "a text with spaces"), ("XY", "Z", ""), ("XA", "A", "!")]))
    recs.append(sh.tiny("ml", 1, 800, seq=_seq(77), tags=[("MM", "Z", "C+m," + ",".join(str(k % 9) for k in range(2496)) + ";"), ("ML", "B", ("C", [k % 256 for k in range(5000)]))]))
    return recs


def _limits_case():
    recs = [sh.tiny("a", 0, -1, flag=0, seq="", cigar=[]), sh.tiny("q" * 254, 1, 0, flag=65535), sh.tiny("z", 0, BIG - 1, flag=4, tlen=BIG, pnext=BIG, rnext="c2"),
            sh.tiny("y", 1, 5, tlen=-BIG, rnext="=", pnext=1), sh.tiny("x", -1, -1, flag=4, rnext="*", seq="ACG", cigar=[]), sh.tiny("w", 0, 7, rnext="c1", pnext=9, seq=_seq(9), qual=_qual(9)),
            sh.tiny("v", 1, 7, seq="", cigar=[(0, 5)]), sh.tiny("u", 0, 7, seq="acgtnNrykmswbdhvXZ.=*-", cigar=[(4, 22)]), sh.tiny("t", 0, 70000, seq="ACGTA", qual="!~#$%"),
            sh.tiny("s", 0, 9, seq="A", cigar=[(k, 1 + k) for k in range(9)] + [(0, (1 << 28) - 1), (2, 0)])]
    for r in recs:
        r["mapq"] = 255 if r["name"] in ("a", "z") else 0 if r["name"] == "y" else 60
    return recs


def _target(lines, at, offset):
    """a filler line such that the body has exactly `offset` bytes after it (lines: the body's lines so far, `at`: their bytes)"""
    room = offset - at
    assert room >= 64, (at, offset)
    base = len(sh.sam_line(sh.tiny("fill%d" % len(lines), 0, 5, seq="", cigar=[]), REFS2)) + 1        # with SEQ `*`
    n = room - base + 1                                      # (SEQ of n bases in place of the `*`)
    r = sh.tiny("fill%d" % len(lines), 0, 5, seq="A" * n, cigar=[])
    assert len(sh.sam_line(r, REFS2)) + 1 == room
    return r


def _edges_case():
    """a line break, then a tab, on the last byte of a step, of a wavefront's share and of a tile, and on the first byte of the next"""
    recs, at = [], 0

    def add(r):
        nonlocal at
        recs.append(r)
        at += len(sh.sam_line(r, REFS2)) + 1
    for edge in (STEP, WAVE_BYTES, TILE, 2 * TILE):
        add(_target(recs, at, edge))                         # its line break is byte edge - 1
        add(_target(recs, at, edge + 70))
        add(_target(recs, at, edge + 200 - 11))
        add(sh.tiny("n123456789", 0, 3))                     # the tab behind its name is byte edge + 199 ...
    for edge in (3 * TILE, 4 * TILE):
        add(_target(recs, at, edge + 1))                     # ... a line break on the first byte of a tile
        add(_target(recs, at, edge + 300 - 10))
        add(sh.tiny("m23456789", 0, 3))                      # a tab on byte edge + 299 ...
        add(_target(recs, at, edge + TILE // 2 - 8))
    for edge in (5 * TILE, 6 * TILE):
        add(_target(recs, at, edge - 8))
        add(sh.tiny("t234567" if edge == 5 * TILE else "t2345678", 0, 3))          # the tab on the tile's last byte, then on the next tile's first
    return recs


def _exact(recs, total):
    """recs plus one filler such that the stream (header and records) has exactly `total` bytes"""
    room = total - len(sh.judge_stream(sh.sam_text(REFS2, recs)))
    for l_seq in range(0, 90000):
        name_len = room - 37 - (l_seq + 1) // 2 - l_seq
        if 1 <= name_len <= 200:
            return recs + [sh.tiny("f" * name_len, 0, 77, seq="A" * l_seq, cigar=[])]
    raise AssertionError("no filler for %d bytes" % room)


def _case(name):
    """-> dict(records | text, refs, and what sam_to_bam is told)"""
    if name[1:].isdigit():
        return dict(records=_plain(int(name[1:]), seed=int(name[1:]) + 1))
    if name == "limits":
        return dict(records=_limits_case())
    if name == "tags":
        return dict(records=_tags_case())
    if name == "residues":                                   # line lengths of every residue 1 .. 129 around the mark pass's 64 x 16 bytes
        return dict(records=[sh.tiny("r%d" % k, k % 2, 10 + k, seq="A" * k, cigar=[]) for k in range(1, 130)])
    if name == "edges":
        return dict(records=_edges_case())
    if name == "lseq":                                       # l_seq 0 .. 130 under names of 1 .. 16 bytes: the nibble tail, and SEQ and QUAL at every alignment mod 16
        return dict(records=[sh.tiny("abcdefghijklmnop"[: 1 + (k * 7 + j) % 16], 0, 100 + k, seq=_seq(k, j), qual=_qual(k, j) if (k + j) % 5 else "*", tags=[("NM", k)][: k % 2])
                             for k in range(131) for j in range(2)])
    if name in ("cg65535", "cg65536", "long"):
        n_ops = dict(cg65535=65535, cg65536=65536, long=70000)[name]
        cigar = [((0, 1), (1, 2), (0, 3), (2, 1))[k % 4] for k in range(n_ops)]
        n_q = sum(ln for op, ln in cigar if op in (0, 1))
        big = sh.tiny("long_read", 0, 25000, seq=_seq(n_q, 5), qual=_qual(n_q, 5) if name == "long" else "*", cigar=cigar, tags=[("NM", 12), ("de", "f", "0.0317")])
        small = _plain(40, seed=12)
        return dict(records=small[:20] + [big] + small[20:])
    if name in ("edge0", "edge1"):                           # the stream ends on a block boundary / one byte past it
        return dict(records=_exact(_plain(300, seed=13, qual=False), 2 * sh.BLOCK + int(name[-1])))
    if name == "carry":                                      # records of about 30 KB: a block's bytes are carried across three one-line windows
        return dict(records=[sh.tiny("c%d" % k, 0, 100 + k, seq=_seq(20000 + k, k), qual=_qual(20000 + k, k), cigar=[(0, 20000 + k)]) for k in range(9)])
    if name == "floats":                                     # 40 fast and 10 slow floats
        texts = [FAST_FLOATS[k % len(FAST_FLOATS)] for k in range(40)] + [SLOW_FLOATS[k % len(SLOW_FLOATS)] for k in range(10)]
        order = np.random.default_rng(3).permutation(50)
        return dict(records=[sh.tiny("f%d" % k, 0, 10 + k, tags=[("NM", k), ("de", "f", texts[int(order[k])])]) for k in range(50)])
    if name == "names300":                                   # names that share long prefixes, one a prefix of another, beyond 64 bytes
        stem = "chrUn_a_very_long_shared_prefix_that_goes_on_and_on_beyond_sixty_four_bytes_"
        refs = [(stem[: 10 + (k % 3) * 30] + "%03d" % ((k * 37) % 300), 1000 + k) for k in range(299)] + [(stem[:40], 77)]
        assert len(set(n for n, _ in refs)) == 300
        rng = np.random.default_rng(8)
        return dict(refs=refs, records=[sh.tiny("r%d" % k, int(rng.integers(0, 300)), 5, rnext=refs[int(rng.integers(0, 300))][0] if k % 3 else "=", pnext=4) for k in range(400)])
    if name == "no_newline":
        return dict(text=sh.sam_text(REFS2, _plain(30, seed=4))[:-1])
    if name == "header_only":
        return dict(text=sh.sam_text(REFS2, []))
    if name == "no_hd":
        return dict(text=sh.sam_text(REFS2, _plain(5, seed=5), hd=False, extra="@CO\ta comment\twith tabs\n@PG\tID:aligner\n"))
    if name == "only_sq":
        return dict(text=sh.sam_text(REFS2, _plain(5, seed=6), hd=False))
    if name == "no_sq_no_lines":
        return dict(text=b"@HD\tVN:1.6\n@CO\tnothing here\n")
    if name == "empty":
        return dict(text=b"")
    raise KeyError(name)


COUNTS = ["n1", "n63", "n64", "n65", "n4097"]
HEADERS = ["header_only", "no_hd", "only_sq", "no_sq_no_lines", "empty", "names300"]
CASES = COUNTS + ["limits", "tags", "residues", "edges", "lseq", "cg65535", "cg65536", "long", "edge0", "edge1", "carry", "floats", "no_newline"] + HEADERS
WINDOWS = dict(carry=1, long=4096, n65=1, edges=5000)        # cases that are also run with small windows: one line each / a window that must grow


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> dict(path, text, want (the judge's stream), host (the host route's file bytes), stats): made once"""
    d = tmp_path_factory.mktemp("sam_input")
    memo = {}

    def get(name):
        if name not in memo:
            c = _case(name)
            text = c["text"] if "text" in c else sh.sam_text(c.get("refs", REFS2), c["records"])
            path, out = str(d / (name + ".sam")), str(d / (name + ".host.bam"))
            with open(path, "wb") as f:
                f.write(text)
            stats = sam.sam_to_bam(path, out, route="host", threads=3)
            with open(out, "rb") as f:
                host = f.read()
            memo[name] = dict(path=path, text=text, want=sh.judge_stream(text), host=host, host_path=out, stats=stats, dir=d, n=len(c["records"]) if "records" in c else None, case=c)
        return memo[name]
    return get


# ------------------------------------------------------------------------------------------------ CPU 1: the core under the sanitizers
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_core")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/sam_core_main.cpp")
    exe = str(d / "sam_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "sam_core_main.cpp")], check=True, capture_output=True, text=True)

    def run(*args):
        p = subprocess.run([exe] + list(args), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout
    return run, d


def test_the_core_under_the_sanitizers_numbers_bases_and_types(core):
    run, _ = core
    out = run("numbers").split()
    assert out[:2] == ["numbers", "ok"] and int(out[2]) > 10000 and int(out[4]) > 1000


@pytest.mark.parametrize("name", ["limits", "tags", "lseq", "cg65536", "no_newline", "no_hd", "names300", "empty"])
def test_the_core_under_the_sanitizers_writes_the_judges_stream(core, built, name):
    run, d = core
    c = built(name)
    out = str(d / (name + ".stream"))
    assert run("stream", c["path"], out).split()[0] == "ok"
    with open(out, "rb") as f:
        assert f.read() == c["want"]
    for w in (1, 4096):
        cuts = [tuple(int(x) for x in ln.split()) for ln in run("windows", c["path"], str(w)).splitlines()]
        head = len(sh.split_header(c["text"])[0])
        assert [a for a, _ in cuts] == [head] + [b for _, b in cuts[:-1]] if cuts else head == len(c["text"])
        assert not cuts or cuts[-1][1] == len(c["text"])


# ------------------------------------------------------------------------------------------------ CPU 2: the host route against the judge
@pytest.mark.parametrize("name", CASES)
def test_the_host_route_writes_the_judges_stream(built, name):
    c = built(name)
    assert sh.inflate_file(c["host_path"]) == c["want"]
    blocks = sh.check_file(c["host"], c["want"])
    st = c["stats"]
    assert st["stream_bytes"] == len(c["want"]) and st["out_bytes"] == len(c["host"]) and st["blocks"] == len(blocks) and st["text_bytes"] == len(c["text"])
    if c["n"] is not None:
        assert st["records"] == c["n"] and st["lines"] == c["n"] + len(sh.split_header(c["text"])[0].splitlines())


def test_the_conventions_written_out(built):
    """what the judge and the code agree on, against bytes written out here: no rule is checked only against its restatement"""
    text = b"@SQ\tSN:c1\tLN:9\n" + b"r\t16\tc1\t0\t7\t*\t=\t5\t-3\tAcN\t*\tXI:i:-129\tde:f:0.5\n"
    rec, counts = sam.records(text[15:], ["c1"])
    want = (bytes([0, 0, 0, 0]) + b"\xff\xff\xff\xff" + bytes([2, 7]) + (4680).to_bytes(2, "little") + bytes([0, 0, 16, 0]) + (3).to_bytes(4, "little") + bytes(4) + (4).to_bytes(4, "little") +
            (-3).to_bytes(4, "little", signed=True) + b"r\0" + bytes([0x12, 0xF0]) + b"\xff\xff\xff" + b"XIs" + (-129).to_bytes(2, "little", signed=True) + b"def" + bytes([0, 0, 0, 0x3F]))
    assert rec == len(want).to_bytes(4, "little") + want and counts == dict(lines=1, float_patches=0, cg_records=0)
    assert sh.judge_stream(text)[-len(rec):] == rec


def test_counts_of_floats_outside_the_fast_path_and_of_cg_records(built):
    assert built("floats")["stats"]["float_patches"] == 10
    assert built("cg65535")["stats"]["cg_records"] == 0 and built("cg65536")["stats"]["cg_records"] == 1 and built("long")["stats"]["cg_records"] == 1
    n_f = len(SLOW_FLOATS) + len(HOST_FLOATS) + sum(t in SLOW_FLOATS for t in (FAST_FLOATS + SLOW_FLOATS)[:1]) + sum(t in SLOW_FLOATS for t in (FAST_FLOATS + SLOW_FLOATS + FAST_FLOATS * 4)[:65])
    assert built("tags")["stats"]["float_patches"] == n_f


def test_the_project_reads_what_the_host_route_wrote(built, tmp_path):
    recs = sorted(_plain(200, seed=31), key=lambda r: (r["refid"], r["start"]))
    path, out = str(tmp_path / "s.sam"), str(tmp_path / "s.bam")
    with open(path, "wb") as f:
        f.write(sh.sam_text(REFS2, recs))
    sam.sam_to_bam(path, out, route="host")
    with bam.BamFile(out, _any_order=True) as bf:
        assert bf.references == ["c1", "c2"] and [int(x) for x in bf.lengths] == [100000, 80000] and bf.sort_order == "unsorted"
        for refid, chrom in enumerate(bf.references):
            mine = [r for r in recs if r["refid"] == refid]
            cols = [bam.decode_host(ch) for ch in bf.chunks(chrom)]
            for key, field in (("ref_start", "start"), ("flag", "flag"), ("mapq", "mapq")):
                assert np.concatenate([c[key] for c in cols]).tolist() == [r[field] for r in mine], key
            assert np.concatenate([c["query_len"] for c in cols]).tolist() == [len(r["seq"]) for r in mine]
            assert np.concatenate([c["cigar"] for c in cols]).tolist() == [ln << 4 | op for r in mine for op, ln in r["cigar"]]
    big = [r for r in built("cg65536")["case"]["records"] if r["name"] == "long_read"]
    with open(path, "wb") as f:
        f.write(sh.sam_text(REFS2, big))
    sam.sam_to_bam(path, out, route="host", overwrite=True)
    with bam.BamFile(out, _any_order=True) as bf:                  # the reader undoes the CG form
        cols = [bam.decode_host(ch) for ch in bf.chunks("c1")]
        assert [np.diff(c["cig_off"]).tolist() for c in cols] == [[65536]] and cols[0]["cigar"].tolist() == [ln << 4 | op for op, ln in big[0]["cigar"]]


# ------------------------------------------------------------------------------------------------ CPU 3: refusals
GOOD = "r\t0\tc1\t5\t60\t4M\t*\t0\t0\tACGT\t*"
BAD_LINES = {
    "fields": ("r\t0\tc1\t5\t60\t4M\t*\t0\t0\tACGT", "fewer than 11 fields"),
    "empty_field": ("r\t0\tc1\t5\t60\t4M\t*\t0\t0\t\t*", "empty field"),
    "empty_tag": (GOOD + "\t", "empty field"),
    "empty_line": ("", "is empty"),
    "cr": (GOOD + "\r", "carriage return"),
    "header": ("@CO\tlate", "header line"),
    "qname": ("q" * 255 + GOOD[1:], "QNAME"),
    "flag_text": (GOOD.replace("\t0\tc1", "\t1x\tc1"), "no decimal number"),
    "flag_sign": (GOOD.replace("\t0\tc1", "\t+1\tc1"), "no decimal number"),
    "flag_range": (GOOD.replace("\t0\tc1", "\t65536\tc1"), "outside its field's range"),
    "mapq_range": (GOOD.replace("\t60\t", "\t256\t"), "outside its field's range"),
    "pos_range": (GOOD.replace("\t5\t60", "\t2147483648\t60"), "outside its field's range"),
    "tlen_range": (GOOD.replace("\t0\t0\tACGT", "\t0\t-2147483648\tACGT"), "outside its field's range"),
    "digits": (GOOD.replace("\t5\t60", "\t0000000000000000005\t60"), "no decimal number"),
    "rname": (GOOD.replace("c1", "c3"), "reference the header lacks"),
    "rnext": (GOOD.replace("\t*\t0\t0", "\tc9\t0\t0"), "reference the header lacks"),
    "cigar_no_op": (GOOD.replace("4M", "4M3"), "bad CIGAR"),
    "cigar_no_len": (GOOD.replace("4M", "M"), "bad CIGAR"),
    "cigar_op": (GOOD.replace("4M", "4Q"), "bad CIGAR"),
    "cigar_len": (GOOD.replace("4M", "268435456M"), "bad CIGAR"),
    "cigar_digits": (GOOD.replace("4M", "0000000004M"), "bad CIGAR"),
    "qual_len": (GOOD[:-1] + "III", "QUAL whose length"),
    "qual_byte": (GOOD[:-1] + "II I", "QUAL byte below 33"),
    "tag_short": (GOOD + "\tXX:i", "TAG:TYPE:VALUE"),
    "tag_colon": (GOOD + "\tXXi:1:", "TAG:TYPE:VALUE"),
    "tag_type": (GOOD + "\tXX:Q:1", "TAG:TYPE:VALUE"),
    "tag_a": (GOOD + "\tXX:A:ab", "TAG:TYPE:VALUE"),
    "tag_h": (GOOD + "\tXX:H:ABC", "TAG:TYPE:VALUE"),
    "tag_h_digit": (GOOD + "\tXX:H:AG", "TAG:TYPE:VALUE"),
    "tag_b_sub": (GOOD + "\tXX:B:x,1", "TAG:TYPE:VALUE"),
    "tag_b_comma": (GOOD + "\tXX:B:C1", "TAG:TYPE:VALUE"),
    "tag_i_text": (GOOD + "\tXX:i:1.5", "no decimal number"),
    "tag_i_high": (GOOD + "\tXX:i:4294967296", "tag value outside its type"),
    "tag_i_low": (GOOD + "\tXX:i:-2147483649", "tag value outside its type"),
    "tag_b_range": (GOOD + "\tXX:B:C,1,256", "tag value outside its type"),
    "tag_b_neg": (GOOD + "\tXX:B:S,-1", "tag value outside its type"),
    "tag_b_empty": (GOOD + "\tXX:B:c,1,,2", "no decimal number"),
    "tag_f_text": (GOOD + "\tXX:f:1.5x", "no decimal number"),
    "tag_bf_text": (GOOD + "\tXX:B:f,1.5,abc", "no decimal number"),
}


def _refused_text(bad, at=3, n=6):
    lines = [GOOD.replace("r\t", "r%d\t" % k) for k in range(n)]
    for k, b in (bad if isinstance(bad, list) else [(at, bad)]):
        lines[k] = b
    return sh.header_text(REFS2).encode() + "".join(ln + "\n" for ln in lines).encode()


@pytest.mark.parametrize("which", sorted(BAD_LINES))
def test_every_refusal_names_its_line_and_writes_nothing(tmp_path, which):
    line, why = BAD_LINES[which]
    path = str(tmp_path / "bad.sam")
    with open(path, "wb") as f:
        f.write(_refused_text(line))
    with pytest.raises(sam.SamError, match="line 7 ") as e:                           # three header lines, three good lines
        sam.sam_to_bam(path, str(tmp_path / "out.bam"), route="host", threads=2)
    assert why in str(e.value)
    assert os.listdir(tmp_path) == ["bad.sam"]
    with pytest.raises(sam.SamError, match="line 7 ") as e2:
        sam.records(_refused_text(line)[len(sh.header_text(REFS2)):], ["c1", "c2"], first_line=4)
    assert str(e2.value) in str(e.value)


def test_the_lowest_of_two_bad_lines_wins_on_every_thread_count_and_window(tmp_path):
    text = _refused_text([(150, BAD_LINES["tag_i_high"][0]), (40, BAD_LINES["cigar_op"][0]), (290, BAD_LINES["fields"][0])], n=300)
    path = str(tmp_path / "bad.sam")
    with open(path, "wb") as f:
        f.write(text)
    for threads, wb in ((1, None), (7, None), (16, 1), (3, 2000)):
        with pytest.raises(sam.SamError, match="line 44 has a bad CIGAR"):
            sam.sam_to_bam(path, str(tmp_path / "out.bam"), route="host", threads=threads, window_bytes=wb)
        assert os.listdir(tmp_path) == ["bad.sam"]                                    # a later window's refusal removes what earlier ones wrote


@pytest.mark.parametrize("which,why", [("dup", "twice"), ("no_sq", "no @SQ line"), ("no_ln", "needs SN and an LN"), ("no_sn", "needs SN and an LN"), ("ln_zero", "needs SN and an LN")])
def test_header_refusals(tmp_path, which, why):
    head = dict(dup="@SQ\tSN:c1\tLN:5\n@SQ\tSN:c2\tLN:5\n@SQ\tSN:c1\tLN:6\n", no_sq="@HD\tVN:1.6\n", no_ln="@SQ\tSN:c1\n", no_sn="@SQ\tLN:5\n", ln_zero="@SQ\tSN:c1\tLN:0\n")[which]
    path = str(tmp_path / "h.sam")
    with open(path, "w") as f:
        f.write(head + GOOD + "\n")
    with pytest.raises(sam.SamError, match=why):
        sam.sam_to_bam(path, str(tmp_path / "o.bam"), route="host")
    assert os.listdir(tmp_path) == ["h.sam"]


# ------------------------------------------------------------------------------------------------ CPU 4: windows, files, command lines
@pytest.mark.parametrize("name", ["n65", "carry", "long", "edges", "no_newline"])
def test_the_file_does_not_depend_on_the_window_on_the_host_route(built, tmp_path, name):
    c = built(name)
    for wb in (1, 4096, None):
        out = str(tmp_path / ("w%s.bam" % wb))
        st = sam.sam_to_bam(c["path"], out, route="host", window_bytes=wb, threads=4)
        with open(out, "rb") as f:
            assert f.read() == c["host"]
        if wb == 1 and c["n"]:
            assert st["windows"] == c["n"]


def test_an_existing_target_is_kept_unless_overwriting_is_asked_for(built, tmp_path):
    c = built("n65")
    out = str(tmp_path / "out.bam")
    with open(out, "wb") as f:
        f.write(b"mine")
    with pytest.raises(FileExistsError):
        sam.sam_to_bam(c["path"], out, route="host")
    with open(out, "rb") as f:
        assert f.read() == b"mine"
    sam.sam_to_bam(c["path"], out, route="host", overwrite=True)
    with open(out, "rb") as f:
        assert f.read() == c["host"]
    assert os.listdir(tmp_path) == ["out.bam"]
    with pytest.raises(ValueError):
        sam.sam_to_bam(c["path"], out, route="gpu", overwrite=True)
    with pytest.raises(ValueError):
        sam.sam_to_bam(c["path"], out, route="host", overwrite=True, window_bytes=0)


def test_is_sam_decides_by_content(built, tmp_path):
    assert sam.is_sam(built("n65")["path"]) and sam.is_sam(built("no_hd")["path"]) and not sam.is_sam(built("n65")["host_path"]) and not sam.is_sam(built("empty")["path"])
    for k, (blob, want) in enumerate([(b"read1\t0\n", True), (b"@", True), (b"\x1f\x8b\x08", False), (b"\x00abc", False), (b" r", False), (b"CRAM", True)]):
        p = str(tmp_path / ("f%d" % k))
        with open(p, "wb") as f:
            f.write(blob)
        assert sam.is_sam(p) == want, blob


def test_the_command_line_of_the_sam_module(built, tmp_path, capsys):
    c = built("n65")
    out = str(tmp_path / "cl.bam")
    assert sam.main([c["path"], "-o", out, "--route", "host"]) == 0
    with open(out, "rb") as f:
        assert f.read() == c["host"]
    assert "65 records" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        sam.main([c["path"], "-o", out, "--route", "host"])
    with pytest.raises(SystemExit):
        sam.main([c["path"]])
    assert sam.main([c["path"], "-o", out, "--route", "host", "--force", "--threads", "2"]) == 0


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted BAM of the calling tests, the same records shuffled as BAM and as SAM text, the reference"""
    d = tmp_path_factory.mktemp("sam_planted")
    path, shuffled, text = str(d / "planted.bam"), str(d / "shuffled.bam"), str(d / "shuffled.sam")
    ref = call_helpers.write_planted_bam(path)
    recs, _ = call_helpers.planted_records()
    mixed = sort_helpers.keep_ties_permutation(recs, seed=21)
    bam_writer.write_bam(shuffled, call_helpers.CONTIGS, mixed, sort_order="unsorted")
    with open(text, "wb") as f:
        f.write(sh.sam_text(call_helpers.CONTIGS, mixed))
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return path, shuffled, text, fa


def test_sort_bam_takes_sam_text_and_writes_the_file_the_bam_input_gives(planted, tmp_path, capsys):
    path, shuffled, text, _ = planted
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    bam.sort_bam(shuffled, a, route="host")
    st = bam.sort_bam(text, b, route="host")
    with open(a, "rb") as f, open(b, "rb") as g:
        assert f.read() == g.read()
    assert st["sam"]["records"] == st["records"] > 40 and st["sam"]["route"] == "host" and sorted(os.listdir(tmp_path)) == ["a.bam", "b.bam"]
    assert sh.inflate_file(b) == sh.inflate_file(path)
    assert bam.main([text, "--sort", "-o", str(tmp_path / "c.bam"), "--sort_route", "host"]) == 0
    with open(a, "rb") as f, open(str(tmp_path / "c.bam"), "rb") as g:
        assert f.read() == g.read()
    with pytest.raises(ValueError, match="not a BGZF block|not a BAM file"):                           # without the sort: today's refusal, in today's words
        bam.BamFile(text)
    assert cli.sorted_input_path("w", "/x/y/reads.sam") == os.path.join("w", "reads.sorted.bam") == cli.sorted_input_path("w", "/x/y/reads.bam")


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _device(ctx, c, out, **kw):
    st = sam.sam_to_bam(c["path"], out, ctx=ctx, route="device", **kw)
    with open(out, "rb") as f:
        return st, f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_the_device_route_writes_the_judges_stream_and_the_host_routes_file(ctx, built, tmp_path, name):
    c = built(name)
    out = str(tmp_path / "dev.bam")
    st, blob = _device(ctx, c, out)
    assert sh.inflate_file(out) == c["want"]
    assert blob == c["host"]
    for k in ("lines", "records", "header_bytes", "text_bytes", "stream_bytes", "out_bytes", "blocks", "windows", "float_patches", "cg_records"):
        assert st[k] == c["stats"][k], k
    assert st["bytes_up"] >= len(c["text"]) - len(sh.split_header(c["text"])[0]) and st["bytes_down"] >= len(blob) - 28


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_gpu_the_file_does_not_depend_on_the_window(ctx, built, tmp_path, name):
    c = built(name)
    st, blob = _device(ctx, c, str(tmp_path / "w.bam"), window_bytes=WINDOWS[name])
    assert blob == c["host"]
    if WINDOWS[name] == 1:
        assert st["windows"] == c["n"]                                                # one line a window
    if name == "carry":
        assert st["blocks"] == len(c["want"]) // sh.BLOCK + 2 and 3 * 32000 > sh.BLOCK > 2 * 32000       # a block's bytes come from three windows
    if name == "long":
        assert st["windows"] < 60 and max(len(ln) for ln in c["text"].splitlines()) > 200000               # one window grew for the long line


@pytest.mark.gpu
def test_gpu_the_patch_rows_are_the_floats_outside_the_fast_path(ctx, built, tmp_path):
    st, blob = _device(ctx, built("floats"), str(tmp_path / "f.bam"))
    assert st["float_patches"] == 10 and st["windows"] == 1 and blob == built("floats")["host"]


@pytest.mark.gpu
def test_gpu_the_lowest_of_three_refused_lines_in_different_tiles_wins(ctx, tmp_path):
    n = 1500                                                                          # lines of about 42 bytes: 63 KB, two tiles of the mark pass
    for low, why in ((BAD_LINES["qual_byte"][0], "QUAL byte below 33"), (BAD_LINES["cigar_op"][0], "bad CIGAR"), (BAD_LINES["tag_b_range"][0], "outside its type")):
        text = _refused_text([(1400, BAD_LINES["fields"][0]), (300, low), (900, BAD_LINES["qual_byte"][0])], n=n)
        path = str(tmp_path / "bad.sam")
        with open(path, "wb") as f:
            f.write(text)
        with pytest.raises(sam.SamError) as host:
            sam.sam_to_bam(path, str(tmp_path / "h.bam"), route="host")
        for wb in (None, 20000):
            with pytest.raises(sam.SamError) as dev:
                sam.sam_to_bam(path, str(tmp_path / "d.bam"), ctx=ctx, route="device", window_bytes=wb)
            assert str(dev.value) == str(host.value) and "line 304 " in str(dev.value) and why in str(dev.value)
        assert os.listdir(tmp_path) == ["bad.sam"]


@pytest.mark.gpu
def test_gpu_end_to_end_shuffled_sam_text_gives_the_bam_inputs_vcf(ctx, planted, tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("CUTESV_AMD_TRA_GT", raising=False)
    path, shuffled, text, fa = planted
    out = str(tmp_path / "sorted.bam")
    st = bam.sort_bam(text, out, ctx=ctx, route="device", inflate=ctx, frame="device")
    assert st["sam"]["route"] == "device" and sh.inflate_file(out) == sh.inflate_file(path)

    def body(vcf_path):
        with open(vcf_path, "rb") as f:
            return b"".join(ln for ln in f.read().splitlines(True) if not ln.startswith(b"##"))
    wd = str(tmp_path / "work")
    os.mkdir(wd)
    common = ["-s", "3", "--genotype", "--report_readid"]
    assert cli.main([path, fa, str(tmp_path / "a.vcf"), wd] + common) == 0
    with pytest.raises(ValueError, match="not a BGZF block|not a BAM file"):                           # without the option: today's refusal
        cli.main([text, fa, str(tmp_path / "x.vcf"), wd] + common)
    for k, route in enumerate(("device", "host")):
        vcf = str(tmp_path / ("b%d.vcf" % k))
        assert cli.main([text, fa, vcf, wd, "--sort_input", route] + common) == 0
        assert body(vcf) == body(str(tmp_path / "a.vcf")) and body(vcf).count(b"\n") > 3
        err = capsys.readouterr().err
        assert os.listdir(wd) == [] and "sort_input" in err and "sam_to_bam" in err
