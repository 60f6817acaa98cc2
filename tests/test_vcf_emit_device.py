"""GPU tests of the device emitter (csv_vcf_emit_device: k_vcf_plan / k_vcf_len / k_vcf_write over cutesv_amd/csrc/vcf_core.h, DESIGN.md section
38) against the host emitter csv_vcf_emit_ref, byte for byte: the crafted table of tests/vcf_core_helpers.py, the shapes at which the plan
grid, the scan tile and the lanes' loops turn over, both string sources, the recorded cases through the HIP cluster path, AF through the
kernel, capacity and every refusal, the kept text with its deflate and its tabix index, call_bam and the command line."""
import gzip
import re

import numpy as np
import pytest

import call_helpers
import vcf_core_helpers as vh
from cutesv_amd import _abi, bam, bgzf, call, cli, engine, fasta, rebuild, vcf
from cutesv_amd.columns import Params
from test_vcf_core import _rows_of, golden_cases, refusal_cases
from test_vcf_emit import _canon, _first_diff

pytestmark = pytest.mark.gpu
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def crafted():
    return vh.crafted()


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emit") / "planted.bam")
    return path, call_helpers.write_planted_bam(path)


def _same(ctx, t, b, svid=None, prefix=b"", what=""):
    """device against host on one built table -> the device's Out; the rows against the text's own restatement"""
    rc, blob, off = vh.ref_of(t, b)
    assert rc == 0, what
    want, got = vh.run("ref", b, blob, off, svid=svid), vh.run("device", b, blob, off, svid=svid, ctx=ctx, prefix=prefix)
    assert want.rc == 0 and got.rc == 0, (what, got.rc, getattr(got, "error", ""))
    assert got.text == prefix + want.text, "%s: %s" % (what, _first_diff(got.text.decode(), (prefix + want.text).decode()))
    assert got.need == len(prefix) + want.need and np.array_equal(got.svid, want.svid) and got.guard_ok, what
    names, rows = _rows_of(prefix + want.text)
    assert got.n_rows == len(rows) == want.text.count(b"\n") and np.array_equal(got.rows, rows), what
    assert [t.chroms[i] for i in got.name_chrom[:got.n_names].tolist()] == names, what
    return got


# ------------------------------------------------------------------------------------------------ byte for byte
def test_the_kernels_write_the_crafted_table_as_the_host_emitter_does(ctx, crafted):
    starts = ([0] * 5, [9] * 5, [99] * 5, [999] * 5, [9, 99, 999, 0, 9999])
    records = 0
    for i, flags in enumerate(vh.FLAG_SETS):
        for j, sizes in enumerate(vh.SIZE_SETS):
            b = vh.vin(crafted, **flags, **sizes)
            got = _same(ctx, crafted, b, svid=starts[(i + j) % len(starts)], what="%s %s" % (flags, sizes))
            records += got.n_rows
    assert records > 24 * 500


@pytest.mark.parametrize("n_calls", (0, 1, 63, 64, 65, 255, 256, 257, 4097))
def test_the_shapes_where_the_grid_the_scan_tile_and_the_lanes_turn_over(ctx, n_calls):
    t = vh.shaped(n_calls, SHAPES)
    got = _same(ctx, t, vh.vin(t, min_size=0, report_readid=True), what="n_calls %d" % n_calls)
    assert got.n_rows == n_calls
    if n_calls >= 255:
        assert set((got.rows[:, 3] % 4).tolist()) == {0, 1, 2, 3}                 # record starts on every residue mod 4
        lens = {len(c["alt"]) for c in t.calls} | {len(c["rn"]) for c in t.calls}
        assert lens >= set(SHAPES)
    if n_calls == 65:
        for k in (1, 2, 3):
            _same(ctx, t, vh.vin(t, min_size=0, report_readid=True), prefix=b"#" * k + b"\n", what="prefix %d" % k)


def test_a_record_of_200001_ref_bases_and_tables_that_emit_nothing_or_their_last_call(ctx):
    t = vh.Table(["c"], {"c": vh.sequence(200100, 3)})
    s = t.seg(vh.DEL, "c", 0)
    t.call(s, 50, 200000)
    t.call(s, 20, 40)
    got = _same(ctx, t, vh.vin(t, max_size=-1), what="long")
    assert got.rows[:, 2].tolist() == [60, 200050] and got.need > 200001
    t = vh.Table(["c"], {"c": vh.sequence(5000, 3)})
    s = t.seg(vh.DEL, "c", 0)
    for i in range(300):
        t.call(s, 10 + i, 20 if i != 299 else 200)
    assert _same(ctx, t, vh.vin(t, min_size=1000), svid=[5] * 5, what="none").svid.tolist() == [5] * 5
    last = _same(ctx, t, vh.vin(t, min_size=100), svid=[5] * 5, what="last")
    assert last.svid.tolist() == [5, 6, 5, 5, 5] and last.n_rows == 1 and last.text.startswith(b"c\t309\tcuteSV.DEL.5\t")


def test_the_recorded_cases_through_the_hip_cluster_path(ctx):
    n = 0
    for g, st, hb, _, ref, kw in golden_cases():
        res = ctx.cluster_batch(hb)
        host, sv_h = vcf.emit_records(st, hb.segments, res, ref, **kw)
        dev, sv_d = vcf.emit_records(st, hb.segments, res, ref, route="device", ctx=ctx, **kw)
        assert dev == host, "%s %s: %s" % (g["case"], g["flags"], _first_diff(dev, host))
        assert np.array_equal(sv_h, sv_d)
        assert _canon(dev) == _canon(g["text"]), "%s %s" % (g["case"], g["flags"])
        n += 1
    assert n >= 21


def test_af_through_the_kernel(ctx):
    tot = np.arange(1, 257)
    dv = np.concatenate([np.arange(1, s + 1) for s in tot])
    dr = np.concatenate([s - np.arange(1, s + 1) for s in tot])
    t = vh.af_table(dv, dr)
    b = vh.vin(t, genotype=True)
    rc, blob, off = vh.ref_of(t, b)
    want, got = vh.run("ref", b, blob, off), vh.run("device", b, blob, off, ctx=ctx)
    assert rc == 0 and want.rc == 0 and got.rc == 0 and len(dv) == 256 * 257 // 2
    if got.text != want.text:
        w, g = want.text.split(b"\n"), got.text.split(b"\n")
        bad = next(i for i in range(len(w)) if w[i] != g[i])
        raise AssertionError("dv %d dr %d: %r, the host emitter writes %r" % (dv[bad], dr[bad], g[bad], w[bad]))
    assert b";AF=0.0312\t" in got.text and b";AF=0.0187\t" in got.text and b";AF=1.0\t" in got.text


# ------------------------------------------------------------------------------------------------ capacity, refusals
def test_capacity_and_every_refusal_leave_the_guard_and_the_counters(ctx, crafted):
    b = vh.vin(crafted, genotype=True, report_readid=True)
    _, blob, off = vh.ref_of(crafted, b)
    full = vh.run("device", b, blob, off, ctx=ctx, svid=[7] * 5)
    assert full.rc == 0
    short = vh.run("device", b, blob, off, ctx=ctx, svid=[7] * 5, cap=full.need - 1)
    assert short.rc == _abi.E_CAPACITY and short.need == full.need and short.guard_ok and short.svid.tolist() == [7] * 5 and short.n_rows == full.n_rows
    exact = vh.run("device", b, blob, off, ctx=ctx, svid=[7] * 5, cap=full.need)
    assert exact.rc == 0 and exact.text == full.text and exact.guard_ok
    names = []
    for name, b, blob, off in refusal_cases():
        got = vh.run("device", b, blob, off, ctx=ctx, svid=[3] * 5)
        assert got.rc == _abi.E_INVALID and got.guard_ok and got.svid.tolist() == [3] * 5, name
        assert "csv_vcf_emit_device: the calls do not fit their tables" in got.error, name
        names.append(name)
    assert len(names) == 9
    t = vh.Table(["c"], {"c": vh.sequence(100, 1)})
    t.call(t.seg(vh.DUP, "c", 0), 5, 50)
    b = vh.vin(t)
    _, blob, off = vh.ref_of(t, b)
    assert vh.run("device", b, blob, off, ctx=ctx, flags=8).rc == _abi.E_INVALID                     # an unknown flag
    assert vh.run("device", b, blob, off, ctx=ctx).rc == 0                                            # ... and the context goes on


# ------------------------------------------------------------------------------------------------ the kept text
def test_the_kept_text_its_deflate_and_its_index(ctx, tmp_path):
    g, st, hb, _, ref, kw = next(x for x in golden_cases() if x[0]["flags"].get("report_readid"))
    res = ctx.cluster_batch(hb)
    header = vcf.header_text([(c, len(ref[c])) for c in st.chroms], "SAMPLE", ["x"]).encode()
    host, _ = vcf.emit_records(st, hb.segments, res, ref, as_bytes=True, **kw)
    kept, svid = vcf.emit_records(st, hb.segments, res, ref, route="device", ctx=ctx, keep=header, **kw)
    text = header + host
    assert kept.n_bytes == len(text) and kept.fetch() == text and kept.n_records == host.count(b"\n") == int(svid.sum()) > 10
    names, rows = _rows_of(text)
    assert kept.names == names and np.array_equal(kept.rows, rows)
    assert all(o == len(header) or text[o - 1:o] == b"\n" for o in kept.rows[:, 3].tolist())      # the offsets land on line starts
    image, table = bgzf.compress_kept(ctx, kept)
    want_image, want_table = bgzf.compress(text, route="core")
    assert image == want_image and all(np.array_equal(a, b) for a, b in zip(table, want_table))
    assert bgzf.decompress(image) == text and gzip.decompress(image) == text
    # a text of several blocks: the cut rule is compress's
    big_header = header + b"##" + b"x" * 150000 + b"\n"
    kept2, _ = vcf.emit_records(st, hb.segments, res, ref, route="device", ctx=ctx, keep=big_header, **kw)
    with pytest.raises(RuntimeError, match="the kept VCF text is gone"):
        kept.fetch()                                                                              # a second emit invalidates the first handle
    with pytest.raises(RuntimeError, match="the kept VCF text is gone"):
        bgzf.compress_kept(ctx, kept)
    image2, table2 = bgzf.compress_kept(ctx, kept2)
    want2 = bgzf.compress(big_header + host, route="core")
    assert len(table2[0]) >= 4 and image2 == want2[0] and bgzf.decompress(image2) == big_header + host
    try:
        want_tbi = bgzf.tabix_raw(big_header + host, table2)
    except bgzf.BgzfError as e:                                                                   # (records of one position in both orders: refused alike)
        with pytest.raises(bgzf.BgzfError, match=re.escape(str(e))):
            bgzf.tabix_rows_raw(kept2.names, kept2.rows, kept2.n_bytes, table2)
    else:
        assert bgzf.tabix_rows_raw(kept2.names, kept2.rows, kept2.n_bytes, table2) == want_tbi
        assert bgzf.decompress(bgzf.tabix_rows(kept2, table2)) == want_tbi
    # an emit that keeps nothing drops the text as well
    vcf.emit_records(st, hb.segments, res, ref, route="device", ctx=ctx, **kw)
    with pytest.raises(RuntimeError, match="the kept VCF text is gone"):
        kept2.fetch()
    with pytest.raises(engine.CsvError, match="the context keeps no VCF text"):
        ctx._check(vh.lib().csv_vcf_text_fetch(ctx._h, None, 0, vh.C.byref(vh.C.c_int64(0))))


# ------------------------------------------------------------------------------------------------ call_bam: the strings from the kept rebuild
@pytest.mark.parametrize("kw", [dict(), dict(report_readid=True), dict(ignore_sequence=True, report_readid=True), dict(genotype=True, report_readid=True)],
                         ids=["plain", "readid", "ignore_sequence", "genotype"])
def test_call_bam_writes_the_same_text_on_the_device(ctx, planted, monkeypatch, kw):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "alignments")
    path, ref = planted
    kw = dict(kw)
    cp = call.CallParams(Params.ont(min_support=3, genotype=kw.pop("genotype", False)))
    with bam.BamFile(path) as bf:
        want, sv_w = call.call_bam(bf, ref, cp, ctx=ctx, **kw)
        timings = {}
        got, sv_g = call.call_bam(bf, ref, cp, ctx=ctx, emit="device", timings=timings, **kw)
    assert got == want and np.array_equal(sv_g, sv_w) and want.count("\n") >= 5
    assert "SVTYPE=INS" in want and "SVTYPE=BND" in want and (("<INS>" in want) == bool(kw.get("ignore_sequence")))
    assert timings["ms_emit_kernels"] > 0 and "ms_alt_gather" not in timings and list(timings)[-1] == "ms_emit"


def test_the_pool_sources_refuse_a_rebuild_that_was_touched(ctx, planted, monkeypatch):
    path, ref = planted
    cp = call.CallParams(Params.ont(min_support=3))
    seen = []
    real = vcf.emit_records
    monkeypatch.setattr(vcf, "emit_records", lambda *a, **k: (seen.append((a, k)), real(*a, **k))[1])
    with bam.BamFile(path) as bf:
        want, _ = call.call_bam(bf, ref, cp, ctx=ctx, emit="device", report_readid=True)
    (a, k), = seen
    k = dict(k, svid=None)
    assert real(*a, **k)[0] == want                                           # the kept rebuild is still there: the same call again
    # the ALT from the pool, the names from a blob; and the other way round
    t = a[2].trimmed()
    names = rebuild.support_join(ctx, t["support_off"], t["support_sig"])
    assert real(*a, **dict(k, from_pool=None, route="host", ctx=None, ins_alt=call._gather_alt(ctx, a[1], a[2], t), rnames=names))[0] == want
    rebuild.pool_append(ctx, [0], [1], [1], [0], [0])
    with pytest.raises(engine.CsvError, match="csv_seq_alt_gather: the pool, the name pool or the scratch arena changed after the kept rebuild: rebuild again"):
        real(*a, **k)
    with pytest.raises(engine.CsvError, match="csv_name_support_join: the pool, the name pool or the scratch arena changed after the kept rebuild: rebuild again"):
        real(*a, **dict(k, ignore_sequence=True))
    with bam.BamFile(path) as bf:                                              # ... and the context goes on
        assert call.call_bam(bf, ref, cp, ctx=ctx, emit="device", report_readid=True)[0] == want


def _write_fasta(path, ref):
    with open(path, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")


def test_call_bam_with_a_bgzf_reference_and_a_compressed_result(ctx, planted, tmp_path):
    path, ref = planted
    fa = str(tmp_path / "ref.fa")
    _write_fasta(fa, ref)
    with open(fa, "rb") as f:
        image, _ = bgzf.compress(f.read(), route="host")
    with open(fa + ".gz", "wb") as f:
        f.write(image)
    cp = call.CallParams(Params.ont(min_support=3))
    with fasta.opened_reference(fa + ".gz") as zref:
        want, _ = call.call_bam(path, zref, cp, ctx=ctx, report_readid=True)
        for ref_route in ("host", "device"):
            assert call.call_bam(path, zref, cp, ctx=ctx, report_readid=True, emit="device", ref_route=ref_route)[0] == want
    assert want == call.call_bam(path, ref, cp, ctx=ctx, report_readid=True)[0]
    header = vcf.header_text(call_helpers.CONTIGS, "NULL", ["a", "b"]).encode()
    timings = {}
    out, svid = call.call_bam(path, ref, cp, ctx=ctx, report_readid=True, emit="device", bgzf_prefix=header, timings=timings)
    text = header + want.encode()
    assert isinstance(out, call.Compressed) and out.text_bytes == len(text) and out.n_records == want.count("\n") == int(svid.sum())
    assert bgzf.decompress(out.image) == text
    core_image, table = bgzf.compress(text, route="core")
    assert out.image == core_image and bgzf.decompress(out.tbi) == bgzf.tabix_raw(text, table)
    assert list(timings)[-4:] == ["ms_emit", "ms_bgzf_kernels", "ms_bgzf", "ms_tabix"] and timings["ms_bgzf_kernels"] > 0 and timings["ms_emit_kernels"] > 0
    empty, _ = call.call_bam(path, ref, cp, ctx=ctx, chroms=["chrB"], emit="device", bgzf_prefix=header)
    assert bgzf.decompress(empty.image) == header and empty.n_records == 0 and bgzf.decompress(empty.tbi)[:4] == b"TBI\1"


def test_the_command_line_writes_the_same_two_files(planted, tmp_path, capsys, monkeypatch):
    path, ref = planted
    fa = str(tmp_path / "ref.fa")
    _write_fasta(fa, ref)
    (tmp_path / "w").mkdir()
    # (the header carries the command line and the time: one fixed header for both runs, so that the two texts - and with them the
    # compressed blocks the virtual offsets of the indexes count - can be equal at all)
    import time
    real = vcf.header_text
    monkeypatch.setattr(vcf, "header_text", lambda contigs, sample, argv, now=None: real(contigs, sample, ["fixed"], now=time.gmtime(0)))
    outs = {}
    for emit in ("host", "device"):
        out = str(tmp_path / (emit + ".vcf.gz"))
        assert cli.main([path, fa, out, str(tmp_path / "w"), "-s", "3", "--report_readid", "--emit", emit, "--bgzf", "device"]) == 0
        outs[emit] = (bgzf.decompress(open(out, "rb").read()), bgzf.decompress(open(out + ".tbi", "rb").read()))
        records = sum(1 for ln in outs[emit][0].split(b"\n") if ln and not ln.startswith(b"#"))
        assert re.search(r"(\d+) records \(INS", capsys.readouterr().err).group(1) == str(records)          # (on the device route the rows count them)
    assert outs["device"][0] == outs["host"][0] and outs["device"][1] == outs["host"][1] and outs["device"][1][:4] == b"TBI\1"
    assert outs["host"][0].startswith(b"##fileformat=VCFv4.2\n") and outs["host"][0].count(b"SVTYPE=") >= 5 and b"RNAMES=" in outs["host"][0]
