"""The BAM index in call_bam and the command line, on the GPU: the planted two-contig BAM of call_helpers,
rewritten with small blocks and indexed by tests/bai_writer.py.  The index moves starting points and lets a BED run skip what lies
between its regions; the text, the svid counters and the .sigs files must not know."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bai_writer
import call_helpers
import index_helpers as ih
from cutesv_amd import bam, bed, call, cli
from cutesv_amd.columns import Params, TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
T1 = 40000 / 9                                  # the first fractional bound of chrA under the index cut with cut_threads=1 (see heavy_cut)


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _floor_reads():
    """three reads that start exactly on floor(T1) = 4444 and carry a 300-base insertion 1500 bases further on"""
    rng = np.random.default_rng(3)
    ins = call_helpers._bases(rng, 300)
    return [dict(name="floor%d" % k, flag=0, mapq=60, start=int(T1), cigar=[(0, 1500), (1, 300), (0, 1200 + k)],
                 seq=call_helpers._bases(rng, 1500) + ins + call_helpers._bases(rng, 1200 + k), tags=[], refid=1) for k in range(3)]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("indexcall")
    path = str(d / "planted.bam")
    ref = ih.write_planted_small_blocks(path, extra=_floor_reads())
    beds = {}
    for name, text in (("ins", "chrA\t9000\t11000\nchrZ\t5\t500\n"), ("tra", "chrA\t24000\t26000\n"), ("two", "chrA\t9000\t11000\nchrA\t29500\t30500\n")):
        beds[name] = str(d / (name + ".bed"))
        with open(beds[name], "w") as f:
            f.write(text)
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return path, ref, beds, d, fa


def _sigs(d):
    return {t: open(os.path.join(d, t + ".sigs"), "rb").read() for t in TYPES}


@pytest.mark.parametrize("genotype,report_readid,batch", [(False, False, 10_000_000), (True, False, 10_000_000), (True, True, 2000), (False, False, 2000)])
def test_the_same_output_with_and_without_the_index(ctx, planted, tmp_path, genotype, report_readid, batch):
    path, ref, _, _, _ = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=genotype))
    outs = []
    for index in (False, None):
        for inflate in ("host", "device"):
            d = tmp_path / ("sigs_%s_%s" % (index, inflate))
            d.mkdir()
            tm = {}
            with bam.BamFile(path, index=index) as bf:
                assert bf.has_index == (index is None)
                text, svid = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid, tra_gt="alignments" if genotype else None, sigs_dir=str(d),
                                           inflate=inflate, read_stats=tm)
            outs.append((text, svid.tolist(), _sigs(str(d)), tm["compressed_bytes"]))
    assert outs[0][0].count("\n") >= 4 and "SVTYPE=BND" in outs[0][0]
    assert all(o[:3] == outs[0][:3] for o in outs[1:])
    assert outs[2][3] <= outs[0][3]                 # (host route; the device route's one large window holds this whole file, so its totals say nothing)


def test_one_contig_reads_fewer_bytes(ctx, planted):
    path, ref, _, _, _ = planted
    cp = call.CallParams(Params.ont(min_support=3))
    got = []
    for index in (False, None):
        tm = {}
        text, _ = call.call_bam(path, ref, cp, ctx=ctx, chroms=[call_helpers.CONTIGS[1][0]], index=index, read_stats=tm)
        got.append((text, tm["compressed_bytes"]))
    assert got[0][0] == got[1][0] and "SVTYPE=INS" in got[0][0]
    assert 0 < got[1][1] < got[0][1]


@pytest.mark.parametrize("tra_gt,genotype", [("off", False), ("reads_table", True), ("off", True)])
@pytest.mark.parametrize("which,batch", [("ins", 10_000_000), ("two", 10_000_000), ("two", 2000)])
def test_a_bed_run_skips_what_lies_between_its_regions(ctx, planted, tra_gt, genotype, which, batch):
    path, ref, beds, _, _ = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=genotype))
    got = []
    for index in (False, None):
        tm = {}
        text, svid = call.call_bam(path, ref, cp, ctx=ctx, include_bed=beds[which], batch=batch, tra_gt=tra_gt, index=index, read_stats=tm, report_readid=genotype)
        got.append((text, svid.tolist(), tm))
    assert got[0][:2] == got[1][:2] and "SVTYPE=INS" in got[0][0]
    assert 0 < got[1][2]["compressed_bytes"] < got[0][2]["compressed_bytes"]
    assert got[1][2]["n_records"] < got[0][2]["n_records"]
    # a task without regions reads nothing: every task of chrB (the BED names no region there), and with the small batch most of chrA's
    n_chrb = len(call.cut_tasks(call_helpers.CONTIGS[0][1], batch))
    names = sorted(c for c, _ in call_helpers.CONTIGS)
    assert names[1] == "chrB" and got[1][2]["task_records"][-n_chrb:] == [0] * n_chrb and sum(got[0][2]["task_records"][-n_chrb:]) > 0
    regions = bed.load_bed(beds[which])
    with bam.BamFile(path) as bf:
        for (t0, t1), n in zip(call.cut_tasks(call_helpers.CONTIGS[1][1], batch), got[1][2]["task_records"]):
            if len(regions.for_task("chrA", t0, t1)) == 0:
                assert n == 0
            else:
                assert call.task_ranges(bf, "chrA", regions.for_task("chrA", t0, t1), t0, t1)


def test_with_the_alignment_table_every_task_reads_its_whole_range(ctx, planted):
    path, ref, beds, _, _ = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=True))
    bnd = lambda text: [ln for ln in text.splitlines() if "SVTYPE=BND" in ln]      # noqa: E731
    full, _ = call.call_bam(path, ref, cp, ctx=ctx, tra_gt="alignments", index=False)
    got = []
    for index in (False, None):
        tm = {}
        text, _ = call.call_bam(path, ref, cp, ctx=ctx, tra_gt="alignments", include_bed=beds["tra"], index=index, read_stats=tm)
        got.append((text, tm["n_records"]))
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1]
    assert len(bnd(full)) >= 1 and bnd(got[1][0]) == bnd(full) and bnd(full)[0].split("\t")[9].split(":")[0] != "./."


def _heavy_cut(bf):
    """the reference's cut of the planted file with -t 1: the unit is a tenth of the mapped reads, both contigs are heavy and chrA is
    cut into nine parts of 40000 / 9 bases"""
    tasks = call.cut_tasks_index(bf.index_statistics(), dict(zip(bf.references, bf.lengths)), 10_000_000, 1)
    assert [t for t in tasks if t[0] == "chrA"][0] == ("chrA", 0, T1) and T1 != int(T1) and len([t for t in tasks if t[0] == "chrA"]) == 9
    return tasks


@pytest.mark.parametrize("which", [None, "two"])
def test_the_index_cut_equals_the_route_through_the_store(ctx, planted, monkeypatch, which):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "reads_table")
    path, ref, beds, _, _ = planted
    cp = call.CallParams(Params.ont(min_support=3))
    regions = None if which is None else bed.load_bed(beds[which])
    with bam.BamFile(path) as bf, bam.BamFile(path, index=False) as plain:
        tasks = _heavy_cut(bf)
        want = ih.store_route(ctx, plain, ref, cp, regions, tasks)
        got, _ = call.call_bam(bf, ref, cp, ctx=ctx, task_cut="index", cut_threads=1, include_bed=regions)
        uniform, _ = call.call_bam(bf, ref, cp, ctx=ctx, include_bed=regions)
        with pytest.raises(ValueError, match="index"):
            call.call_bam(plain, ref, cp, ctx=ctx, task_cut="index")
    assert got == want and got.count("\n") >= 1
    if which is None:
        # the reads planted on floor(t1) of the fractional bound belong to the task in front of it: their insertion is called
        assert got == uniform
        at = [ln.split("\t") for ln in got.splitlines() if ln.startswith("chrA\t") and abs(int(ln.split("\t")[1]) - (int(T1) + 1500)) <= 5]
        assert len(at) == 1 and "SVTYPE=INS" in at[0][7] and "RE=3" in at[0][7]


@pytest.mark.parametrize("window_blocks", [1, 64])
def test_the_read_grid_on_the_device_inflate(ctx, tmp_path, window_blocks):
    path = str(tmp_path / "grid.bam")
    _, info = ih.write_grid_bam(path)
    W = ih.WINDOW
    with bam.BamFile(path, inflate=ctx) as dev, bam.BamFile(path, index=False) as host:
        dev.set_inflate(ctx, window_blocks=window_blocks)
        n_dev = 0
        for chrom, (_, length), R in zip([r[0] for r in ih.REFS], ih.REFS, info["refs"]):
            for beg, end in list(ih.grid_pairs(ih.grid_points(len(R["ioffset"]), length), length)) + [(-bam.ALL, bam.ALL), (0, length)]:
                a, b = dev.records(chrom, beg, end), host.records(chrom, beg, end)
                assert ih.same_chunk(a, b), (chrom, beg, end)
                n_dev += a.stats["device_blocks"]
                assert a.stats["fallback_blocks"] == 0
            a = dev.records(chrom, ranges=[(5, 900), (12 * W - 90, 12 * W), (44 * W, 46 * W)])
            assert ih.same_chunk(a, host.records(chrom, ranges=[(5, 900), (12 * W - 90, 12 * W), (44 * W, 46 * W)]))
        assert n_dev > 50


def test_the_command_lines(ctx, planted, tmp_path, capsys):
    path, ref, beds, d, fa = planted
    cp = cli.call_params(cli.parse_args([path, fa, "out.vcf", str(tmp_path), "-s", "3", "-t", "1"]))
    with bam.BamFile(path) as bf:
        want, _ = call.call_bam(bf, ref, cp, ctx=ctx, task_cut="index", cut_threads=1, include_bed=beds["two"])
        uniform, _ = call.call_bam(bf, ref, cp, ctx=ctx, include_bed=beds["two"])
    body = lambda p: "".join(ln for ln in open(p) if not ln.startswith("#"))       # noqa: E731
    work = tmp_path / "work"
    work.mkdir()
    args = [path, fa, None, str(work), "-s", "3", "-t", "1", "-include_bed", beds["two"]]
    for extra, text in (([], want), (["--task_cut", "index"], want), (["--task_cut", "uniform"], uniform)):
        args[2] = str(tmp_path / ("out%d.vcf" % len(extra)))
        assert cli.main(args + extra) == 0
        assert body(args[2]) == text
    assert "no BAM index" not in capsys.readouterr().err
    plain = str(tmp_path / "plain.bam")                                    # no index beside it: the uniform cut, and one line says so
    with open(path, "rb") as f, open(plain, "wb") as g:
        g.write(f.read())
    args[0], args[2] = plain, str(tmp_path / "plain.vcf")
    assert cli.main(args) == 0 and body(args[2]) == uniform
    assert capsys.readouterr().err.count("no BAM index") == 1
    with pytest.raises(ValueError, match="index"):
        cli.main(args + ["--task_cut", "index"])
    p = subprocess.run([sys.executable, "-m", "cutesv_amd.bam", path, "--idxstats"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    info = bai_writer.build(open(path, "rb").read())
    assert p.stdout.splitlines() == ["%s\t%d\t%d\t%d" % (c, n, R["n_mapped"], R["n_unmapped"]) for (c, n), R in zip(call_helpers.CONTIGS, info["refs"])] + ["*\t0\t0\t0"]
