"""CPU tests of the record core (cutesv_amd/csrc/vcf_core.h): csv_vcf_emit_core_host - the rule the device emitter's
kernels run, with one lane - against the host emitter csv_vcf_emit / csv_vcf_emit_ref, byte for byte: on the recorded cases of
vcf_lines.json.gz (and against the reference's text), on a crafted table with every branch of a record, on every refusal, over a whole
domain of AF values, as a stand-alone program under the sanitizers; csv_tbx_build_rows against csv_tbx_build; and the emit option of
call_bam and the two command lines."""
import argparse
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vcf_core_helpers as vh
from cutesv_amd import _abi, bgzf, call, cli, synth, vcf
from cutesv_amd.columns import Params
from helpers import load_json, store_from_json
from oracle import oracle
from test_vcf_emit import _canon, _first_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crafted():
    return vh.crafted()


def golden_cases():
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    for g in load_json("vcf_lines.json.gz"):
        case = small[g["case"]]
        st, p = store_from_json(case["store"]), Params(**case["params"])
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        hb = st.host_batch([(t, c) for t, c, _ in case["rows"]], p)
        yield g, st, hb, oracle.cluster_batch(hb, per_sig=False), ref, dict(min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, **g["flags"])


# ------------------------------------------------------------------------------------------------ byte for byte
def test_the_core_writes_the_recorded_cases_as_the_host_emitter_does():
    n = 0
    for g, st, hb, res, ref, kw in golden_cases():
        host, sv_h = vcf.emit_records(st, hb.segments, res, ref, **kw)
        core, sv_c = vcf.emit_records(st, hb.segments, res, ref, route="core", **kw)
        assert core == host, "%s %s: %s" % (g["case"], g["flags"], _first_diff(core, host))
        assert np.array_equal(sv_h, sv_c) and int(sv_c.sum()) == core.count("\n")
        assert _canon(core) == _canon(g["text"]), "%s %s: %s" % (g["case"], g["flags"], _first_diff(_canon(core), _canon(g["text"])))
        n += 1
    assert n >= 21


def test_the_crafted_table_holds_what_it_claims(crafted):
    t = crafted
    b = vh.vin(t, genotype=True, report_readid=True)
    rc, blob, off = vh.ref_of(t, b)
    text = vh.run("ref", b, blob, off).text.decode()
    for what in ("SVTYPE=INS", "SVTYPE=DEL", "SVTYPE=DUP", "SVTYPE=INV", "SVTYPE=BND", "STRAND=++", "STRAND=--", "IMPRECISE", "\tq5\t", "\tPASS\t", ";AF=.", ";AF=0.9688", ";AF=0.0187",
                 "./.:.:", ";RNAMES=;", ";RNAMES=read/", "\tN\t", "N[", "N]", "]N", "[N", ":%d[" % (vh.P31 + 1), "Z" * 40 + "\t", "\nA\t", "\t%d\t" % vh.P31):
        assert what in text, what
    assert rc == 0 and "\nN0\t" not in text and text.index("\nA\t") < text.index("\n" + "Z" * 40) < text.index("\nchrB\t")
    refs = set("".join(re.findall(r"cuteSV\.DEL\.\d+\t([^\t]+)\t", text)))                 # every IUPAC code was met and mapped; lower case passes
    assert refs >= set("ACGTNacgtryswkmbdhvn") and not refs & set("RYSWKMBDHV") and set(re.findall(r"\t([A-Z])\t<DUP>", text)) <= set("ACGTN")
    lens = {len(x) for x in re.findall(r"SVLEN=-?(\d+)", text)}
    assert lens >= {2, 3, 4, 5, 6}


@pytest.mark.parametrize("sizes", range(len(vh.SIZE_SETS)))
def test_the_core_writes_the_crafted_table_as_the_host_emitter_does(crafted, sizes):
    t = crafted
    starts = ([0] * 5, [9] * 5, [99] * 5, [999] * 5, [9, 99, 999, 0, 9999], [99999, 9, 0, 999, 99])
    total = 0
    for i, flags in enumerate(vh.FLAG_SETS):
        b = vh.vin(t, **flags, **vh.SIZE_SETS[sizes])
        rc, blob, off = vh.ref_of(t, b)
        assert rc == 0
        for svid in (starts[i % len(starts)], starts[(i + 3) % len(starts)]):
            want, got = vh.run("ref", b, blob, off, svid=svid), vh.run("core", b, blob, off, svid=svid)
            assert want.rc == 0 and got.rc == 0 and got.guard_ok
            assert got.text == want.text, "%s %s: %s" % (flags, svid, _first_diff(got.text.decode(), want.text.decode()))
            assert got.need == want.need and np.array_equal(got.svid, want.svid) and int((got.svid - np.array(svid)).sum()) == got.text.count(b"\n") > 500
            total += got.text.count(b"\n")
    dropped = [len(t.calls) - vh.run("core", vh.vin(t, **s), *vh.ref_of(t, vh.vin(t, **s))[1:]).text.count(b"\n") for s in vh.SIZE_SETS]
    assert all(d > 100 for d in dropped) and len(set(dropped)) == 3            # every size set drops calls, each its own


# ------------------------------------------------------------------------------------------------ refusals
def _small():
    t = vh.Table(["c", "d"], {"c": vh.sequence(400, 1), "d": vh.sequence(300, 2)})
    sd, si, su, sv, sb = (t.seg(ty, "c", 1) for ty in (vh.DEL, vh.INS, vh.DUP, vh.INV, vh.TRA))
    key = vh.gl_index(10, 10)
    t.call(sd, 10, 50, dr=10, support=10, gl=key)
    t.call(si, 20, 40, dr=10, support=10, gl=key, alt=b"ACGT" * 10)
    t.call(su, 399, 420, dr=10, support=10, gl=key)
    t.call(sv, 100, 200, dr=10, support=10, gl=key, aux=1)
    t.call(sb, 399, 7, dr=10, support=10, gl=key, aux=8 + 2)
    t.call(sd, 30, 5, dr=3, support=1, gl=vh.gl_index(3, 1))                         # dropped by min_size; its genotype row is looked up all the same
    return t


def _refusals():
    """name -> (table as built, mutate(b, blob, off) applied after the REF blob was made)"""
    def seg_out(b, blob, off): b.res.arrays["call_seg"][2] = len(b.segs)
    def seg_neg(b, blob, off): b.res.arrays["call_seg"][0] = -1
    def chrom_out(b, blob, off): b.segs[1]["chrom"] = 2
    def no_row(b, blob, off): b.res.arrays["gl_idx"][0] = vh.gl_index(30, 2)
    def no_row_filtered(b, blob, off): b.res.arrays["gl_idx"][5] = vh.gl_index(30, 2)
    def outside(b, blob, off): b.res.arrays["bp1"][2] = 400
    def short_contig(b, blob, off): b.clen[0] = 399
    def fewer_bytes(b, blob, off): off[1:] -= 1
    def more_bytes(b, blob, off): off[4:] += 1
    return dict(seg_out=seg_out, seg_neg=seg_neg, chrom_out=chrom_out, no_row=no_row, no_row_filtered=no_row_filtered, outside=outside, short_contig=short_contig,
                fewer_bytes=fewer_bytes, more_bytes=more_bytes)


def refusal_cases():
    for name, mutate in _refusals().items():
        t = _small()
        b = vh.vin(t, genotype=True)
        rc, blob, off = vh.ref_of(t, b)
        assert rc == 0
        blob = np.append(blob, np.frombuffer(b"ACGT", np.uint8))
        mutate(b, blob, off)
        yield name, b, blob, off


def test_every_refusal_of_the_host_emitter_is_the_cores_with_nothing_written():
    t = _small()
    b = vh.vin(t, genotype=True)
    _, blob, off = vh.ref_of(t, b)
    ok = vh.run("core", b, blob, off)
    assert ok.rc == 0 and ok.text == vh.run("ref", b, blob, off).text and ok.text.count(b"\n") == 5
    names = []
    for name, b, blob, off in refusal_cases():
        want, got = vh.run("ref", b, blob, off, svid=[3] * 5), vh.run("core", b, blob, off, svid=[3] * 5)
        assert want.rc == got.rc == _abi.E_INVALID, name
        assert got.guard_ok and want.guard_ok and got.svid.tolist() == [3] * 5, name
        names.append(name)
    assert len(names) == 9


def test_one_byte_short_gives_the_exact_need(crafted):
    b = vh.vin(crafted, genotype=True, report_readid=True)
    _, blob, off = vh.ref_of(crafted, b)
    full = vh.run("core", b, blob, off, svid=[7] * 5)
    for entry in ("ref", "core"):
        short = vh.run(entry, b, blob, off, svid=[7] * 5, cap=full.need - 1)
        assert short.rc == _abi.E_CAPACITY and short.need == full.need and short.guard_ok and short.svid.tolist() == [7] * 5, entry
        exact = vh.run(entry, b, blob, off, svid=[7] * 5, cap=full.need)
        assert exact.rc == 0 and exact.text == full.text and exact.guard_ok, entry


# ------------------------------------------------------------------------------------------------ AF
def _af_equal(dv, dr, chunk=1 << 18):
    for lo in range(0, len(dv), chunk):
        t = vh.af_table(dv[lo:lo + chunk], dr[lo:lo + chunk])
        b = vh.vin(t, genotype=True)
        rc, blob, off = vh.ref_of(t, b)
        want, got = vh.run("ref", b, blob, off), vh.run("core", b, blob, off)
        assert rc == 0 and want.rc == 0 and got.rc == 0
        if got.text != want.text:
            w, g = want.text.split(b"\n"), got.text.split(b"\n")
            bad = next(i for i in range(len(w)) if w[i] != g[i])
            raise AssertionError("dv %d dr %d: %r, the host emitter writes %r" % (dv[lo + bad], dr[lo + bad], g[bad], w[bad]))
        assert got.text.count(b";AF=") == len(t.calls)


def test_af_is_printfs_over_the_whole_small_domain():
    """every (dv, dr) with dv >= 1 and dv + dr <= 2048: ties (1/32 is exact: 0.0312) and the values a double lies beside (3/160) included"""
    tot = np.arange(1, 2049)
    dv = np.concatenate([np.arange(1, s + 1) for s in tot])
    dr = np.concatenate([s - np.arange(1, s + 1) for s in tot])
    assert len(dv) == 2048 * 2049 // 2
    _af_equal(dv, dr)
    t = vh.af_table(np.array([1, 3, 1, 5]), np.array([31, 157, 0, 3]))
    b = vh.vin(t, genotype=True)
    text = vh.run("core", b, *vh.ref_of(t, b)[1:]).text.decode()
    assert re.findall(r";AF=([0-9.]+)", text) == ["0.0312", "0.0187", "1.0", "0.625"]


def test_af_is_printfs_on_random_pairs_up_to_2_31():
    rng = np.random.default_rng(20)
    dv = rng.integers(1, 1 << 31, 10000)
    dr = np.where(rng.random(10000) < 0.5, rng.integers(0, 1 << 31, 10000), rng.integers(0, 50, 10000))
    _af_equal(dv, dr)


# ------------------------------------------------------------------------------------------------ the tabix index from rows
def _rows_of(text):
    """the rows csv_vcf_emit_device writes beside a text, restated from the text: name index by first appearance, POS - 1, END when greater, else + len(REF)"""
    names, rows, at = [], [], 0
    for line in text.split(b"\n")[:-1]:
        if not line.startswith(b"#"):
            col = line.split(b"\t")
            if col[0].decode() not in names:
                names.append(col[0].decode())
            beg = int(col[1]) - 1
            m = re.search(rb"(?:^|;)END=(\d+)", col[7])
            end = int(m.group(1)) if m and int(m.group(1)) > beg else beg + len(col[3])
            rows.append((names.index(col[0].decode()), beg, end, at))
        at += len(line) + 1
    return names, np.array(rows, np.int64).reshape(-1, 4)


def _table_cut_at(text, rows):
    """a block table over `text` in which record 3 starts a block and record 5 straddles a boundary; the compressed sizes are made up"""
    cuts = sorted({0, int(rows[3, 3]), int(rows[5, 3]) + 7, len(text) // 2, len(text)} | set(range(0, len(text), 65280)))
    uoff = np.array(cuts, np.int64)
    isize = np.append(np.diff(uoff), 0).astype(np.uint32)
    coff = np.zeros(len(uoff), np.int64)
    coff[1:] = np.cumsum(isize[:-1] // 3 + 26)
    assert int(rows[3, 3]) in cuts and not any(int(rows[5, 3]) == c for c in cuts) and rows[5, 3] < rows[5, 3] + 7 < rows[6, 3]
    return uoff, coff, isize


def _orderable():
    """records of every type whose POS never decreases on a contig, on three contigs"""
    t = vh.Table(["k", "a", "zz"], {"k": vh.sequence(90000, 1), "a": vh.sequence(90000, 2), "zz": vh.sequence(70000, 3)})
    for name in ("a", "zz", "k"):
        segs = [t.seg(ty, name, 0) for ty in (vh.DEL, vh.INS, vh.DUP, vh.INV, vh.TRA)]
        for i in range(60):
            ty = i % 5
            p = 50 + 1000 * i
            t.call(segs[ty], p, [700 * (1 + i % 30), 45, p + 300 + i, p + 2000 * (i % 7), 11][ty], aux=[0, 0, 0, i % 2, 8 * t.chroms.index("a" if name != "a" else "k") + i % 4][ty],
                   alt=b"ACGT" * 11, rn=b"r%d" % i)
    return t


def test_the_index_from_rows_is_the_index_from_the_text(crafted):
    texts = []
    for g, st, hb, res, ref, kw in golden_cases():
        if g["flags"].get("report_readid") or not texts:
            texts.append(vcf.emit_records(st, hb.segments, res, ref, as_bytes=True, **kw)[0])
    t = _orderable()
    b = vh.vin(t, report_readid=True)
    texts.append(b"##fileformat=VCFv4.2\n#CHROM\tPOS\n" + vh.run("core", b, *vh.ref_of(t, b)[1:]).text)
    done = 0
    for text in texts:
        names, rows = _rows_of(text)
        if len(rows) < 8:
            continue
        table = _table_cut_at(text, rows)
        try:
            want = bgzf.tabix_raw(text, table)
        except bgzf.BgzfError as e:
            with pytest.raises(bgzf.BgzfError, match=re.escape(str(e))):
                bgzf.tabix_rows_raw(names, rows, len(text), table)
            continue
        assert bgzf.tabix_rows_raw(names, rows, len(text), table) == want
        done += 1
    assert done >= 2 and len(_rows_of(texts[-1])[1]) == 180
    # the refusals, by ordinal, with the text parser's words: out of order, a contig that reappears, a position at or beyond 2^29
    b = vh.vin(crafted)
    text = vh.run("core", b, *vh.ref_of(crafted, b)[1:]).text
    names, rows = _rows_of(text)
    table = (np.array([0, len(text)], np.int64), np.array([0, 100], np.int64), np.array([len(text), 0], np.uint32))
    seen = set()
    for cut in (slice(0, None), slice(0, 6)):
        sub = rows[cut]
        stop = int(sub[-1, 3]) + text[int(sub[-1, 3]):].index(b"\n") + 1
        for rws, txt in ((sub, text[:stop]),):
            try:
                bgzf.tabix_raw(txt, table)
                continue
            except bgzf.BgzfError as e:
                seen.add(re.sub(r"line \d+ ", "", str(e)))
                with pytest.raises(bgzf.BgzfError, match=re.escape(str(e))):
                    bgzf.tabix_rows_raw(names, rws, len(txt), table)
    lines = [b"a\t5\t.\tA\t<DUP>\t.\tPASS\tEND=9", b"b\t5\t.\tA\t<DUP>\t.\tPASS\tEND=9", b"a\t7\t.\tA\t<DUP>\t.\tPASS\tEND=9", b"c\t%d\t.\tA\t<DUP>\t.\tPASS\tEND=9" % (1 << 29)]
    for pick in ([0, 1, 2], [0, 1, 3], [1, 0, 0], [0, 2, 0]):
        txt = b"".join(lines[i] + b"\n" for i in pick)
        names, rows = _rows_of(txt)
        table = (np.array([0, len(txt)], np.int64), np.array([0, 100], np.int64), np.array([len(txt), 0], np.uint32))
        try:
            want = bgzf.tabix_raw(txt, table)
            assert bgzf.tabix_rows_raw(names, rows, len(txt), table) == want
        except bgzf.BgzfError as e:
            seen.add(re.sub(r"line \d+ ", "", str(e)))
            with pytest.raises(bgzf.BgzfError, match=re.escape(str(e))):
                bgzf.tabix_rows_raw(names, rows, len(txt), table)
    assert len(seen) >= 2, seen


# ------------------------------------------------------------------------------------------------ under the sanitizers
def test_the_core_as_a_stand_alone_program_under_the_sanitizers(crafted, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (the library's own build needs it too)"
    exe = str(tmp_path / "vcf_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread",
                    "-o", exe, os.path.join(ROOT, "tests", "vcf_core_main.cpp"), os.path.join(ROOT, "cutesv_amd", "csrc", "vcf_emit.cpp")], check=True, capture_output=True, text=True)
    for i, (flags, svid) in enumerate(((dict(genotype=True, report_readid=True), [9, 99, 999, 0, 9]), (dict(ignore_sequence=True, max_size=-1), [0] * 5))):
        b = vh.vin(crafted, **flags)
        _, blob, off = vh.ref_of(crafted, b)
        table, out = str(tmp_path / ("t%d.bin" % i)), str(tmp_path / ("t%d.vcf" % i))
        vh.dump(table, crafted, b, blob, off, svid)
        r = subprocess.run([exe, table, out], capture_output=True, text=True)
        want = vh.run("ref", b, blob, off, svid=svid)
        assert r.returncode == 0 and r.stdout.split() == ["ok", str(want.need)] + [str(v) for v in want.svid.tolist()], (r.stdout[-2000:], r.stderr[-2000:])
        assert open(out, "rb").read() == want.text


# ------------------------------------------------------------------------------------------------ options
def test_the_emit_option_of_call_bam_and_of_both_command_lines(monkeypatch, tmp_path):
    assert call.DEFAULT_EMIT == "host" and vcf.DEFAULT_ROUTE == "host"
    p = Params()
    assert call.resolve_options("x.bam", None, p).emit == "host"
    assert call.resolve_options("x.bam", None, p, emit="device").emit == "device" and call.resolve_options("x.bam", None, p, emit="host").emit == "host"
    assert "emit" in [f.name for f in __import__("dataclasses").fields(call.Options)]
    with pytest.raises(ValueError, match="emit must be 'host' or 'device', not 'gpu'"):
        call.resolve_options("x.bam", None, p, emit="gpu")
    # its place in the order of the refusals: behind index_format and ref_route, in front of task_cut and everything after it
    with pytest.raises(ValueError, match="index_format"):
        call.resolve_options("x.bam", None, p, emit="gpu", index_format="tbi")
    with pytest.raises(ValueError, match="ref_route"):
        call.resolve_options("x.bam", None, p, emit="gpu", ref_route="gpu")
    with pytest.raises(ValueError, match="emit must be"):
        call.resolve_options("x.bam", None, p, emit="gpu", task_cut="bogus", reads_table="gpu", frame="gpu")
    with pytest.raises(ValueError, match="bgzf_prefix needs emit='device'"):
        call.call_bam("x.bam", {}, p, bgzf_prefix=b"##h\n")
    with pytest.raises(ValueError, match="route='device' needs ctx"):
        vcf.emit_records(None, None, None, None, route="device")
    with pytest.raises(ValueError, match="route must be one of"):
        vcf.emit_records(None, None, None, None, route="gpu")
    ap = argparse.ArgumentParser()
    call.add_route_options(ap)
    assert ap.parse_args(["--emit", "device"]).emit == "device" and ap.parse_args([]).emit is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--emit", "gpu"])
    ns, rest = cli.split_own(["a", "--emit", "device", "--bgzf", "device", "b"])
    assert (ns.emit, ns.bgzf, rest) == ("device", "device", ["a", "b"]) and cli.split_own(["a"])[0].emit is None
    with pytest.raises(SystemExit):
        cli.split_own(["--emit", "gpu"])
    seen = []
    monkeypatch.setattr(call, "call_bam", lambda *a, **k: (seen.append(k), (b"", np.zeros(5, np.int64)))[1])
    monkeypatch.setattr(call.fasta, "open_reference", lambda path, **kw: type("R", (), dict(close=lambda self: None))())
    assert call.main(["a.bam", "ref.fa", "-o", str(tmp_path / "o.vcf"), "--emit", "device"]) == 0 and seen[-1]["emit"] == "device"
    assert call.main(["a.bam", "ref.fa", "-o", str(tmp_path / "o.vcf")]) == 0 and seen[-1]["emit"] is None
