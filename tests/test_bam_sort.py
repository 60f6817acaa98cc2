"""Coordinate-sorting a BAM file: cutesv_amd.bam.sort_bam, csv_bam_sort / csv_bam_sort_host, sort_core.h.

The judge is tests/sort_helpers.py's independent restatement - Python's stable sort on (refid as unsigned, pos, reverse bit) over the
records of the input's inflated stream, its own reading of the header rule - never the twin alone and never the code under test.
CPU: the core under the sanitizers (tests/sort_core_main.cpp), the host route on every case, the header rule, the command lines, the
refusals.  GPU: the device route on every reader route - host inflate, device inflate, device inflate with device framing - against
the judge and against the host route's file, byte for byte."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bai_writer
import bam_writer
import call_helpers
import sort_helpers as sh
from cutesv_amd import bam, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS2 = [("c1", 100000), ("c2", 80000)]
BIG = (1 << 31) - 1
READERS = ("host", "inflate", "frame")                     # the reader routes: host inflate, device inflate, device inflate + device framing


# ------------------------------------------------------------------------------------------------ the cases
def _exact(refs, recs, total, sort_order="unsorted"):
    """recs plus one filler record such that the SORTED stream (its header says SO:coordinate) has exactly `total` bytes"""
    text = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)).encode()
    have = len(sh.header_bytes(text, refs)) + sum(len(bam_writer.record_bytes(r)[0]) for r in recs)
    room = total - have
    for l_seq in range(0, 40000):
        name_len = room - 37 - (l_seq + 1) // 2 - l_seq
        if 1 <= name_len <= 200:
            return recs + [sh.tiny("f" * name_len, 0, 77, seq="A" * l_seq)]
    raise AssertionError("no filler for %d bytes" % room)


def _case(name):
    """-> dict(refs, records, and what write_bam / sort_bam are told)"""
    if name[1:].isdigit():                                   # record counts at the wavefront edge and at SORT_WTILE
        return dict(refs=REFS2, records=sh.random_tiny(int(name[1:]), seed=int(name[1:]) + 1))
    if name == "names":                                      # every name length 1 .. 17: source and destination meet at every alignment mod 16
        rng = np.random.default_rng(4)
        recs = [sh.tiny("abcdefghijklmnopq"[:ln], int(rng.integers(0, 2)), int(rng.integers(0, 9000)), flag=int(rng.choice([0, 16])))
                for rep in range(9) for ln in range(1, 18)]
        return dict(refs=REFS2, records=[recs[i] for i in rng.permutation(len(recs))])
    if name == "blocks97":                                   # records straddle BGZF blocks everywhere
        return dict(refs=REFS2, records=sh.random_tiny(400, seed=9), block_bytes=97)
    if name == "cuts":                                       # block ends inside the block_size word and inside the fixed fields
        return dict(refs=REFS2, records=sh.random_tiny(300, seed=10), cuts="fields")
    if name == "windows":                                    # records straddle reader windows of two blocks
        return dict(refs=REFS2, records=sh.random_tiny(1500, seed=11), block_bytes=211, window_blocks=2)
    if name == "big":                                        # one record of about 105 KB - three output blocks - between tiny ones
        recs = sh.random_tiny(60, seed=12)
        big = sh.tiny("long_read", 0, 25000, seq="ACGT" * 17500, cigar=[(0, 70000)])
        return dict(refs=REFS2, records=recs[:30] + [big] + recs[30:])
    if name in ("edge0", "edge1"):                           # the sorted stream ends on a block boundary / one byte past it
        return dict(refs=REFS2, records=_exact(REFS2, sh.random_tiny(2500, seed=13), 2 * sh.BLOCK + int(name[-1])))
    if name == "four":                                       # four output blocks: the slices
        return dict(refs=REFS2, records=sh.random_tiny(4000, seed=14, name="read_number_%d"))
    if name == "ties":                                       # 200 records on three positions, both strands, distinct names
        rng = np.random.default_rng(15)
        return dict(refs=REFS2, records=[sh.tiny("t%03d" % i, 0, int(rng.choice([500, 501, 9000])), flag=int(rng.choice([0, 16]))) for i in range(200)])
    if name == "wide":                                       # refid -1 scattered, pos -1 on a real contig, positions across 2^29 up to 2^31 - 2, 300 @SQ lines
        rng = np.random.default_rng(16)
        refs = [("s%d" % i, BIG if i in (0, 299) else 1000) for i in range(300)]
        recs = []
        for i in range(900):
            k = i % 9
            if k == 0:
                recs.append(sh.tiny("u%d" % i, -1, -1, flag=4))
            elif k == 1:
                recs.append(sh.tiny("m%d" % i, int(rng.choice([0, 150, 299])), -1, flag=4))
            elif k < 5:
                recs.append(sh.tiny("p%d" % i, int(rng.choice([0, 299])), int(rng.choice([(1 << 29) - 1, 1 << 29, (1 << 29) + 1, (1 << 30) + 5, BIG - 1, 0, 7])), flag=int(rng.choice([0, 16]))))
            else:
                recs.append(sh.tiny("r%d" % i, int(rng.integers(0, 300)), int(rng.integers(0, 1000)), flag=int(rng.choice([0, 16]))))
        return dict(refs=refs, records=recs, raw=True)
    if name in ("sorted", "reversed"):                       # distinct keys, in order and in reverse
        recs = [sh.tiny("k%d" % i, i // 400, 3 * (i % 400) + 1, flag=0) for i in range(800)]
        return dict(refs=REFS2, records=recs if name == "sorted" else recs[::-1], sort_order="coordinate" if name == "sorted" else "unsorted")
    raise KeyError(name)


COUNTS = ["n0", "n1", "n2", "n63", "n64", "n65", "n4095", "n4096", "n4097"]
CASES = COUNTS + ["names", "blocks97", "cuts", "windows", "big", "edge0", "edge1", "four", "ties", "wide", "sorted", "reversed"]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> dict(path, stream (inflated input), want (the judge's stream), host (the host route's file bytes), stats, kw): made once"""
    d = tmp_path_factory.mktemp("bam_sort")
    memo = {}

    def get(name):
        if name not in memo:
            c = _case(name)
            path = str(d / (name + ".bam"))
            kw = {k: c[k] for k in ("block_bytes", "sort_order") if k in c}
            kw.setdefault("sort_order", "unsorted")
            if c.get("raw"):                                 # (positions bam_writer's bin field cannot take: the records are patched, the stream written as it is)
                text = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in c["refs"])).encode()
                sh.write_stream(path, sh.header_bytes(text, c["refs"]) + b"".join(sh.raw_record(r) for r in c["records"]), block_bytes=4001)
            else:
                info = bam_writer.write_bam(path, c["refs"], c["records"], **kw)
            if c.get("cuts") == "fields":
                cuts = [r["offset"] + (2 if i % 2 else 0) + (0 if i % 3 else 11) + (i % 5 == 0) * 19 for i, r in enumerate(info["records"])]
                bam_writer.write_bam(path, c["refs"], c["records"], cuts=cuts, **kw)
            stream = sh.inflate_file(path)
            want = sh.judge(stream)[0]
            out = str(d / (name + ".host.bam"))
            sort_kw = {k: c[k] for k in ("window_blocks",) if k in c}
            stats = bam.sort_bam(path, out, route="host", **sort_kw)
            with open(out, "rb") as f:
                host = f.read()
            memo[name] = dict(path=path, stream=stream, want=want, host=host, host_path=out, stats=stats, kw=sort_kw, dir=d, n=len(c["records"]))
        return memo[name]
    return get


def _check_file(blob, want):
    blocks = sh.blocks_of(blob)
    assert all(size <= 65536 and isize <= sh.BLOCK for _, size, isize in blocks)
    assert blob[-28:] == bam_writer.EOF_BLOCK and blocks[-1][2] == 0
    assert [isize for _, _, isize in blocks[:-1]] == [min(sh.BLOCK, len(want) - a) for a in range(0, len(want), sh.BLOCK)]
    return blocks


# ------------------------------------------------------------------------------------------------ CPU 1: the core
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_core")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/sort_core_main.cpp")
    exe = str(d / "sort_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "sort_core_main.cpp")], check=True, capture_output=True, text=True)

    def run(*args):
        p = subprocess.run([exe] + list(args), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout
    return run, d


def test_the_core_under_the_sanitizers_keys_and_refusals(core):
    run, _ = core
    rows = [[int(x) for x in ln.split()] for ln in run("keys").splitlines()]
    assert len(rows) == 10 * 9 * 5
    for refid, pos, flag, n_ref, why, key in rows:
        want_why = 1 if not -1 <= refid < n_ref else 2 if pos < -1 else 0
        assert why == want_why, (refid, pos)
        if not why:
            assert key == ((n_ref if refid < 0 else refid) << 33 | (pos + 1) << 1 | ((flag >> 4) & 1)), (refid, pos, flag)
    ok = sorted((r for r in rows if not r[4]), key=lambda r: r[5])                 # the key's order is the judge's order
    assert [(r[0] & 0xFFFFFFFF, r[1], (r[2] >> 4) & 1) for r in ok] == sorted((r[0] & 0xFFFFFFFF, r[1], (r[2] >> 4) & 1) for r in ok)


def test_the_core_under_the_sanitizers_tile_rule_on_every_tile_size(core):
    run, _ = core
    out = run("tiles").split()
    assert out[:2] == ["tiles", "ok"] and int(out[2]) > 100000


HEADER_TEXTS = {
    "unsorted": b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n@PG\tID:aligner\n",
    "queryname": b"@HD\tVN:1.6\tSO:queryname\tGO:query\tSS:queryname:natural\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n",
    "no_so": b"@HD\tVN:1.5\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n",
    "no_hd": b"@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n@CO\t@HD is not here\n",
    "empty": b"",
}
HEADER_WANT = {
    "unsorted": b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n@PG\tID:aligner\n",
    "queryname": b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n",
    "no_so": b"@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n",
    "no_hd": b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:80000\n@CO\t@HD is not here\n",
    "empty": b"@HD\tVN:1.6\tSO:coordinate\n",
}


@pytest.mark.parametrize("which", sorted(HEADER_TEXTS))
def test_the_header_rule_in_the_core_and_on_the_host_route(core, which, tmp_path):
    run, _ = core
    head = sh.header_bytes(HEADER_TEXTS[which], REFS2)
    want = sh.header_bytes(HEADER_WANT[which], REFS2)
    assert sh.judge_header(head) == want                                           # (the judge's rule, against the texts written out above)
    src, dst = str(tmp_path / "in.hdr"), str(tmp_path / "out.hdr")
    with open(src, "wb") as f:
        f.write(head)
    assert run("header", src, dst).split()[0] == "ok"
    with open(dst, "rb") as f:
        assert f.read() == want
    recs = b"".join(bam_writer.record_bytes(r)[0] for r in sh.random_tiny(40, seed=3))
    path, out = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    sh.write_stream(path, head + recs, block_bytes=500)
    st = bam.sort_bam(path, out, route="host")
    got = sh.inflate_file(out)
    assert got == sh.judge(head + recs)[0] and got.startswith(want) and st["records"] == 40
    with bam.BamFile(out) as bf:
        assert bf.sort_order == "coordinate" and bf.references == ["c1", "c2"]


# ------------------------------------------------------------------------------------------------ CPU 2: the host route on every case
@pytest.mark.parametrize("name", CASES)
def test_the_host_route_writes_the_judges_stream(built, name):
    c = built(name)
    assert sh.inflate_file(c["host_path"]) == c["want"]
    blocks = _check_file(c["host"], c["want"])
    st = c["stats"]
    assert st["records"] == c["n"] and st["inversions"] == sh.inversions(c["stream"]) and st["inflated_bytes"] == len(c["stream"])
    assert st["stream_bytes"] == len(c["want"]) and st["out_bytes"] == len(c["host"]) and st["blocks"] == len(blocks)
    uoff, coff, isize = st["block_table"]
    assert [(int(a), int(b)) for a, b in zip(coff, isize)] == [(o, i) for o, _, i in blocks] and int(uoff[-1]) == len(c["want"])


def test_an_input_in_order_has_no_inversions_and_a_reversed_one_all_of_them(built):
    a, b = built("sorted"), built("reversed")
    assert a["stats"]["inversions"] == 0 and b["stats"]["inversions"] == b["n"] - 1
    assert sh.split_stream(sh.inflate_file(a["host_path"]))[1] == sh.split_stream(a["stream"])[1]
    assert sh.inflate_file(b["host_path"]) == sh.inflate_file(a["host_path"])


def test_ties_keep_input_order_and_the_tails_sort_as_the_rule_says(built):
    recs = sh.split_stream(sh.inflate_file(built("ties")["host_path"]))[1]
    order = [(struct.unpack_from("<i", r, 8)[0], (struct.unpack_from("<H", r, 18)[0] >> 4) & 1, int(r[37:40])) for r in recs]
    assert order == sorted(order) and len(set(o[:2] for o in order)) == 6          # position, forward before reverse, then the input's order
    recs = sh.split_stream(sh.inflate_file(built("wide")["host_path"]))[1]
    refid = [struct.unpack_from("<i", r, 4)[0] for r in recs]
    k = refid.index(-1)
    assert k > 0 and set(refid[k:]) == {-1} and len(refid) - k == 100
    assert [int(r[37 : r.index(b"\0", 36)]) for r in recs[k:]] == list(range(0, 900, 9))      # the tail: in input order
    first = {}
    for r in recs[:k]:
        first.setdefault(struct.unpack_from("<i", r, 4)[0], struct.unpack_from("<i", r, 8)[0])
    assert first[150] == -1 and first[0] == -1 and first[299] == -1                # pos -1 comes first on its contig
    assert max(struct.unpack_from("<i", r, 8)[0] for r in recs) == BIG - 1


def test_slices_do_not_change_the_file_on_the_host_route(built, tmp_path):
    c = built("four")
    assert c["stats"]["blocks"] == 5 and c["stats"]["slices"] == 1
    for sb in (1, 2):
        out = str(tmp_path / ("s%d.bam" % sb))
        st = bam.sort_bam(c["path"], out, route="host", slice_blocks=sb)
        assert st["slices"] == (4 + sb - 1) // sb
        with open(out, "rb") as f:
            assert f.read() == c["host"]


# ------------------------------------------------------------------------------------------------ CPU 3: refusals, budget, files, command lines
def _patched(built, tmp_path, field_off, value, ordinal=17):
    c = built("n65")
    head, recs = sh.split_stream(c["stream"])
    r = bytearray(recs[ordinal])
    struct.pack_into("<i", r, field_off, value)
    recs[ordinal] = bytes(r)
    path = str(tmp_path / "patched.bam")
    sh.write_stream(path, head + b"".join(recs), block_bytes=333)
    return path


@pytest.mark.parametrize("what", ["refid", "pos"])
def test_a_record_without_a_place_in_the_order_is_refused_by_ordinal(built, tmp_path, what):
    path = _patched(built, tmp_path, 4, 2) if what == "refid" else _patched(built, tmp_path, 8, -2)
    out = str(tmp_path / "out.bam")
    with pytest.raises(bam.BamError, match=r"cannot sort: record 17 has a (refID outside -1 \.\. 1|pos below -1)") as e:
        bam.sort_bam(path, out, route="host")
    assert ("refID" in str(e.value)) == (what == "refid")
    assert os.listdir(tmp_path) == ["patched.bam"]                                 # nothing is written, nothing is left behind


def test_the_budget_refusal_names_both_numbers_and_writes_nothing(built, tmp_path):
    c = built("four")
    out = str(tmp_path / "out.bam")
    need = len(c["stream"]) + 2 * sh.BLOCK
    with pytest.raises(bam.BamError, match="cannot sort") as e:
        bam.sort_bam(c["path"], out, route="host", max_bytes=need - 1, slice_blocks=2)
    assert str(need) in str(e.value) and str(need - 1) in str(e.value) and "samtools sort" in str(e.value)
    assert os.listdir(tmp_path) == []
    assert bam.sort_bam(c["path"], out, route="host", max_bytes=need, slice_blocks=2)["records"] == c["n"]


def test_an_existing_target_is_kept_unless_overwriting_is_asked_for(built, tmp_path):
    c = built("n65")
    out = str(tmp_path / "out.bam")
    with open(out, "wb") as f:
        f.write(b"mine")
    with pytest.raises(FileExistsError):
        bam.sort_bam(c["path"], out, route="host")
    with open(out, "rb") as f:
        assert f.read() == b"mine"
    bam.sort_bam(c["path"], out, route="host", overwrite=True, index="bai")
    with open(out, "rb") as f:
        assert f.read() == c["host"]
    assert sorted(os.listdir(tmp_path)) == ["out.bam", "out.bam.bai"]
    with pytest.raises(bam.BamError, match="SO:unsorted"):                         # the default has not moved: BamFile refuses the input as before
        bam.BamFile(c["path"])
    with pytest.raises(ValueError):
        bam.sort_bam(c["path"], out, route="gpu", overwrite=True)


def test_the_project_reads_what_the_host_route_wrote(built):
    c = built("n4097")
    with bam.BamFile(c["host_path"], index=False) as bf:
        st = bf.build_index()                                                      # (the index build refuses any record out of order)
        assert st["records"] == c["n"] and bf.sort_order == "coordinate"
        info = bai_writer.build(c["host"])
        assert bf.index_bytes() == bai_writer.to_bytes(info)
        assert sum(bf.count(r) for r in bf.references + [None]) == c["n"]


def test_the_command_line_of_the_bam_module_sorts(built, tmp_path, capsys):
    c = built("n65")
    out = str(tmp_path / "cl.bam")
    assert bam.main([c["path"], "--sort", "-o", out, "--sort_route", "host", "--index"]) == 0
    with open(out, "rb") as f:
        assert f.read() == c["host"]
    assert os.path.exists(out + ".bai") and "65 records" in capsys.readouterr().out
    for argv in ([c["path"], "--sort"], [c["path"], "-o", out], [c["path"], "--sort", "-o", out, "--sort_route", "host", "--frame", "device", "--inflate", "device"],
                 [c["path"], "--sort", "-o", out, "--sort_route", "host"], [c["path"], "--sort", "-o", out, "--chrom", "c1"], [c["path"], "--max_bytes", "5"]):
        with pytest.raises(SystemExit):
            bam.main(argv)
    with open(out, "rb") as f:
        assert f.read() == c["host"]
    assert bam.main([c["path"], "--sort", "-o", out, "--sort_route", "host", "--force", "--max_bytes", "100000000"]) == 0


def test_sort_input_is_an_own_option_of_the_calling_command_line(tmp_path):
    own, rest = cli.split_own(["a.bam", "--sort_input", "device", "ref.fa", "-s", "3"])
    assert own.sort_input == "device" and rest == ["a.bam", "ref.fa", "-s", "3"]
    assert cli.split_own(["a.bam"])[0].sort_input is None and cli.split_own(["--sort_input", "host"])[0].sort_input == "host"
    with pytest.raises(SystemExit):
        cli.split_own(["--sort_input", "gpu"])
    assert cli.sorted_input_path("w", "/x/y/reads.bam") == os.path.join("w", "reads.sorted.bam")


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _device(ctx, c, out, reader, **kw):
    routes = dict(host={}, inflate=dict(inflate=ctx), frame=dict(inflate=ctx, frame="device"))[reader]
    st = bam.sort_bam(c["path"], out, ctx=ctx, route="device", **routes, **dict(c["kw"], **kw))
    with open(out, "rb") as f:
        return st, f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("name", CASES)
def test_gpu_the_device_route_writes_the_judges_stream_and_the_host_routes_file(ctx, built, tmp_path, name, reader):
    c = built(name)
    out = str(tmp_path / "dev.bam")
    st, blob = _device(ctx, c, out, reader)
    assert sh.inflate_file(out) == c["want"]
    _check_file(blob, c["want"])
    assert blob == c["host"]
    hs = c["stats"]
    for k in ("records", "inversions", "inflated_bytes", "stream_bytes", "out_bytes", "blocks", "slices"):
        assert st[k] == hs[k], k
    assert st["frame"] == ("device" if reader == "frame" else "host") and st["inflate"] == ("host" if reader == "host" else "device")
    assert all(int(a) == int(b) for x, y in zip(st["block_table"], hs["block_table"]) for a, b in zip(x, y))
    if name == "wide":
        assert st["passes"] >= 6                                                   # the refid digit spans two passes above the position's


@pytest.mark.gpu
@pytest.mark.parametrize("reader", READERS)
def test_gpu_slices_do_not_change_the_file(ctx, built, tmp_path, reader):
    c = built("four")
    for sb in (1, 2):
        st, blob = _device(ctx, c, str(tmp_path / ("s%d.bam" % sb)), reader, slice_blocks=sb)
        assert st["slices"] == (4 + sb - 1) // sb and blob == c["host"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["refid", "pos"])
def test_gpu_refusals_are_the_host_routes_by_ordinal_and_text(ctx, built, tmp_path, what):
    path = _patched(built, tmp_path, 4, 2) if what == "refid" else _patched(built, tmp_path, 8, -2)
    with pytest.raises(bam.BamError) as host:
        bam.sort_bam(path, str(tmp_path / "h.bam"), route="host")
    for reader in READERS:
        with pytest.raises(bam.BamError) as dev:
            _device(ctx, dict(path=path, kw={}), str(tmp_path / "d.bam"), reader)
        assert str(dev.value) == str(host.value) and "cannot sort: record 17 " in str(dev.value)
    assert os.listdir(tmp_path) == ["patched.bam"]


@pytest.mark.gpu
def test_gpu_the_budget_is_checked_before_anything_is_read(ctx, built, tmp_path):
    c = built("four")
    need = len(c["stream"]) + sh.BLOCK
    with pytest.raises(bam.BamError) as e:
        _device(ctx, c, str(tmp_path / "o.bam"), "frame", max_bytes=need - 1, slice_blocks=1)
    assert str(need) in str(e.value) and str(need - 1) in str(e.value) and os.listdir(tmp_path) == []


@pytest.mark.gpu
def test_gpu_the_project_reads_what_the_device_route_wrote(ctx, built, tmp_path):
    c = built("n4097")
    out = str(tmp_path / "o.bam")
    st, blob = _device(ctx, c, out, "frame", index="bai")
    assert st["index"]["records"] == c["n"]
    with open(out + ".bai", "rb") as f:
        assert f.read() == bai_writer.to_bytes(bai_writer.build(blob))
    with bam.BamFile(out, inflate=ctx, frame="device") as bf:
        assert bf.has_index and bf.sort_order == "coordinate" and sum(bf.count(r) for r in bf.references + [None]) == c["n"]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted BAM of the calling tests, and the same records shuffled so that equal keys keep their order"""
    d = tmp_path_factory.mktemp("sort_planted")
    path, shuffled = str(d / "planted.bam"), str(d / "shuffled.bam")
    ref = call_helpers.write_planted_bam(path)
    recs, _ = call_helpers.planted_records()
    bam_writer.write_bam(shuffled, call_helpers.CONTIGS, sh.keep_ties_permutation(recs, seed=21), sort_order="unsorted")
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return path, shuffled, fa


@pytest.mark.gpu
def test_gpu_end_to_end_an_unsorted_input_gives_the_sorted_inputs_vcf(ctx, planted, tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("CUTESV_AMD_TRA_GT", raising=False)
    path, shuffled, fa = planted
    assert sh.inversions(sh.inflate_file(shuffled)) > 10
    out = str(tmp_path / "sorted.bam")
    bam.sort_bam(shuffled, out, ctx=ctx, route="device", inflate=ctx, frame="device")
    assert sh.inflate_file(out) == sh.inflate_file(path)                           # the original file's stream, header and all

    def body(vcf_path):
        with open(vcf_path, "rb") as f:
            return b"".join(ln for ln in f.read().splitlines(True) if not ln.startswith(b"##"))
    wd = str(tmp_path / "work")
    os.mkdir(wd)
    common = ["-s", "3", "--genotype", "--report_readid"]
    assert cli.main([path, fa, str(tmp_path / "a.vcf"), wd] + common) == 0
    with pytest.raises(bam.BamError, match="SO:unsorted"):                         # without the option: today's refusal
        cli.main([shuffled, fa, str(tmp_path / "x.vcf"), wd] + common)
    assert cli.main([shuffled, fa, str(tmp_path / "b.vcf"), wd, "--sort_input", "device"] + common) == 0
    assert body(str(tmp_path / "a.vcf")) == body(str(tmp_path / "b.vcf")) and body(str(tmp_path / "a.vcf")).count(b"\n") > 3
    assert os.listdir(wd) == [] and "sort_input" in capsys.readouterr().err
    assert cli.main([shuffled, fa, str(tmp_path / "c.vcf"), wd, "--sort_input", "device", "--retain_work_dir", "--inflate", "device", "--frame", "device"] + common) == 0
    assert os.listdir(wd) == ["shuffled.sorted.bam"] and body(str(tmp_path / "c.vcf")) == body(str(tmp_path / "a.vcf"))
    assert sh.inflate_file(os.path.join(wd, "shuffled.sorted.bam")) == sh.inflate_file(path)
