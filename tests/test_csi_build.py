"""The CSI index built on the device: build_index(format="csi") with device inflate and device framing - the
index kernels under the file's own binning scheme, k_index_loff for the per-bin loffsets, the linear arrays never downloaded - against
the host route and tests/csi_writer.py, payload byte for byte, at every window size; the refusals on every route; the byte counter;
the built index at work; and call_bam with a built or a found .csi against the .bai run."""
import os
import shutil

import pytest

import bai_writer
import csi_helpers as ch
import csi_writer as cw
import frame_helpers as fh
import index_helpers as ih
from cutesv_amd import bam, call, cli
from cutesv_amd.columns import Params

FILES = ("edges_auto", "edges_14_6", "edges_12_7", "spans_14_6", "spans_12_6", "counts_14_6", "counts_14_5", "three_refs", "big_grid")
WINDOWS = (1, 2, 64, 0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{name: (path, (min_shift, depth or None), csi_writer's info)} of every file of the comparison, written once"""
    d = tmp_path_factory.mktemp("csi_build")
    out = {}
    for name, path, fmt in ch.build_files(d):
        min_shift, depth = fmt or (14, None)
        with open(path, "rb") as f:
            info = cw.build(f.read(), min_shift, depth)
        info["payload"] = cw.to_payload(info)
        out[name] = (path, (min_shift, depth), info)
    assert tuple(out) == FILES
    return out


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def _framed(ctx, path, wb=0, **kw):
    bf = bam.BamFile(path, threads=2, inflate=ctx, frame="device", **kw)
    if wb:
        bf.set_inflate(ctx, window_blocks=wb)
        bf.set_frame("device")
    return bf


def _window_records(path, wb):
    """the records of every window the reader forms at `wb` blocks"""
    stream, lens = fh.stream_of(path)
    return [len(fh.naive_walk(w, c)[0]) for w, _, c in fh.windows_of(stream, lens, wb or 4096)]


def _n_pairs(info):
    return sum(len(R["bins"]) for R in info["refs"])


def _seam_rows(path, info, wb):
    """run rows a device build hands down: the writer's chunks, plus one for every window whose first record carries on the run of the
    record before it"""
    recs, n, extra = info["records"], 0, 0
    key = lambda r: (r["refid"], cw.reg2bin(max(r["pos"], 0), max(r["end"], 1), info["min_shift"], info["depth"]))       # noqa: E731
    for k in _window_records(path, wb):
        if 0 < n < len(recs) and recs[n]["refid"] >= 0 and key(recs[n]) == key(recs[n - 1]):
            extra += 1
        n += k
    return sum(len(c) for R in info["refs"] for c in R["bins"].values()) + extra


# ------------------------------------------------------------------------------------------------ CPU: the files, and the host route
def test_the_files_hold_what_their_names_say(files):
    path, fmt, info = files["edges_auto"]
    assert info["depth"] == 6 and sorted(r["pos"] for r in info["records"] if r["refid"] == 0) == [ch.P29 - 1] * 3 + [ch.P29, ch.P29 + 7, (1 << 31) - 2]
    assert (info["refs"][0]["n_unmapped"], info["n_no_coor"]) == (2, 2)
    assert files["edges_12_7"][2]["depth"] == 7
    for name, shift in (("spans_14_6", 14), ("spans_12_6", 12)):
        recs = [r for r in files[name][2]["records"] if r["refid"] == 0]
        assert [((r["end"] - 1) >> shift) - (r["pos"] >> shift) + 1 for r in recs] == [1, 4, 5, 68, 70]           # windows a record touches
    for name in ("counts_14_6", "counts_14_5"):
        assert _window_records(files[name][0], 1)[:5] == list(ch.COUNTS), name                                   # records per index window
    info = files["three_refs"][2]
    assert [R["n_mapped"] for R in info["refs"]] == [20, 0, 20, 20] and len(info["records"]) < 64                 # one wavefront
    assert cw.level_of(max(files["big_grid"][2]["refs"][0]["bins"]), 6) == 6 and min(files["big_grid"][2]["refs"][0]["bins"]) < cw.first(4)


@pytest.mark.parametrize("name", FILES)
def test_host_payload_equals_the_writers(files, name):
    path, (min_shift, depth), info = files[name]
    with bam.BamFile(path, index=False) as bf:
        st = bf.build_index(format="csi", min_shift=min_shift, depth=depth)
        assert bf.index_payload() == info["payload"] and st["bytes_down"] == 0 and st["records"] == len(info["records"])
        assert bf.index_format == "csi"


# ================================================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", FILES)
def test_gpu_device_payload_equals_host_equals_the_writers(ctx, files, name):
    path, (min_shift, depth), info = files[name]
    kw = dict(format="csi", min_shift=min_shift, depth=depth)
    with bam.BamFile(path, index=False) as bf:
        bf.build_index(**kw)
        host, host_file = bf.index_payload(), bf.index_bytes()
    assert host == info["payload"]
    with bam.BamFile(path, inflate=ctx, index=False) as bf:                   # device inflate + host framing
        st = bf.build_index(**kw)
        assert bf.index_payload() == host and st["inflate"] == "device" and st["frame"] == "host"
    for wb in WINDOWS:
        with _framed(ctx, path, wb, index=False) as bf:
            st = bf.build_index(**kw)
            assert bf.index_payload() == host and bf.index_bytes() == host_file, (name, wb)
            assert st["frame"] == "device" and st["records"] == len(info["records"]) and bf.index_format == "csi"
            want = [(n, R["n_mapped"], R["n_unmapped"], R["n_mapped"] + R["n_unmapped"]) for n, R in zip(bf.references, info["refs"])]
            assert bf.index_statistics() == want and bf.no_coordinate == info["n_no_coor"]
            # what comes down: a status byte per block, the verdicts, the run rows, 8 bytes per bin, the counts - and no linear array
            assert st["runs"] == _seam_rows(path, info, wb), (name, wb, st)
            assert st["bytes_down"] == (st["device_blocks"] + st["fallback_blocks"] + 32 * st["frame_runs"] + 32 * st["index_windows"] + 32 * st["runs"]
                                        + 8 * (_n_pairs(info) + 2 * len(bf.lengths) + 1)), (name, wb, st)
            assert st["bins"] == _n_pairs(info) and (st["ms_loff"] > 0) == (st["bins"] > 0)
            assert st["fallback_blocks"] == 0 and st["frame_fallback_blocks"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ch.REFUSALS))
def test_gpu_refusals_are_the_same_on_every_route(ctx, tmp_path, name):
    refs, recs, (min_shift, depth), ordinal, text = ch.REFUSALS[name]
    path = str(tmp_path / (name + ".bam"))
    ch.write_bam(path, refs, recs, block_bytes=300)
    kw = dict(format="csi", min_shift=min_shift, depth=depth, write=True)
    texts = []
    for open_it in (lambda: bam.BamFile(path, index=False), lambda: bam.BamFile(path, inflate=ctx, index=False), lambda: _framed(ctx, path, 0, index=False),
                    lambda: _framed(ctx, path, 1, index=False)):
        with open_it() as bf:
            with pytest.raises(bam.BamError) as ei:
                bf.build_index(**kw)
            texts.append(str(ei.value))
            assert not bf.has_index and sum(bf.count(c) for c in bf.references) >= 1
    assert len(set(texts)) == 1 and "cannot build the index: record %d %s" % (ordinal, text) in texts[0], texts
    assert os.listdir(tmp_path) == [os.path.basename(path)]


@pytest.mark.gpu
def test_gpu_the_built_index_is_at_work(ctx, files):
    path, _, info = files["big_grid"]
    recs = ch.big_records()
    with _framed(ctx, path, 0, index=False) as ix, bam.BamFile(path, index=False) as fw:
        ix.build_index(format="csi")
        assert ix.has_index and ix.index_format == "csi"
        n = ix.records("also", 580_000_000, 580_000_001)                       # on the device routes: a direct seek
        assert n.n == 1 and n.stats["compressed_bytes"] < fw.records("also", 580_000_000, 580_000_001).stats["compressed_bytes"] / 4
        ix.set_frame(None)                                                      # the index stays when the routes change
        ix.set_inflate(None)
        ch.check_read_grid(ix, fw, recs)


# ------------------------------------------------------------------------------------------------ call_bam
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the planted BAM with small blocks three times: with the .bai beside it, with only a .csi, and alone"""
    d = tmp_path_factory.mktemp("csi_call")
    with_bai, with_csi, without = str(d / "with.bam"), str(d / "csi.bam"), str(d / "without.bam")
    ref = ih.write_planted_small_blocks(with_bai)
    shutil.copy(with_bai, with_csi)
    shutil.copy(with_bai, without)
    cw.write_csi(with_csi)
    bed = str(d / "two.bed")
    with open(bed, "w") as f:
        f.write("chrA\t9000\t11000\nchrA\t29500\t30500\n")
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return with_bai, with_csi, without, ref, bed, fa, d


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("bed", [False, True])
def test_gpu_call_bam_with_a_csi_found_or_built_equals_the_bai_run(ctx, planted, route, bed):
    with_bai, with_csi, without, ref, bed_path, _, d = planted
    cp = call.CallParams(Params.ont(min_support=3))
    kw = dict(ctx=ctx, task_cut="index", cut_threads=1, include_bed=bed_path if bed else None, frame=route, tra_gt="off" if bed else None)
    outs = []
    for path, extra in ((with_bai, {}), (with_csi, {}), (without, dict(index="build", index_format="csi"))):
        rs = {}
        text, svid = call.call_bam(path, ref, cp, read_stats=rs, **extra, **kw)
        outs.append((text, svid.tolist(), rs["task_records"]))
    assert outs[0] == outs[1] == outs[2] and outs[0][0].count("\n") >= 1
    assert sorted(os.listdir(d)) == ["csi.bam", "csi.bam.csi", "ref.fa", "two.bed", "with.bam", "with.bam.bai", "without.bam"]      # nothing was written
    with bam.BamFile(with_csi) as bf:
        assert bf.index_format == "csi"


@pytest.mark.gpu
def test_gpu_the_command_lines(planted, tmp_path, capsys):
    with_bai, with_csi, without, ref, bed_path, fa, d = planted
    body = lambda p: "".join(ln for ln in open(p) if not ln.startswith("#"))       # noqa: E731
    work = tmp_path / "work"
    work.mkdir()
    args = [None, fa, None, str(work), "-s", "3", "-t", "1", "-include_bed", bed_path]
    outs = {}
    for name, path, extra in (("bai", with_bai, []), ("csi", with_csi, []), ("built", without, ["--build_index", "--index_format", "csi", "--frame", "device"])):
        args[0], args[2] = path, str(tmp_path / (name + ".vcf"))
        assert cli.main(args + extra) == 0
        outs[name] = (body(args[2]), capsys.readouterr().err)
    assert outs["bai"][0] == outs["csi"][0] == outs["built"][0] and outs["bai"][0].count("\n") >= 1
    assert "uniform cut" not in outs["csi"][1] and "one is built in memory" in outs["built"][1]
    dev = str(tmp_path / "dev.csi")
    assert bam.main([without, "--index", "--csi", "--index_out", dev, "--inflate", "device", "--frame", "device"]) == 0
    assert bai_writer.read_blocks(open(dev, "rb").read())[1] == cw.write_csi(without, str(tmp_path / "w.csi"))["payload"] and "frame device" in capsys.readouterr().out
    own, rest = cli.split_own(["a.bam", "--build_index", "--index_format", "csi", "ref.fa"])
    assert own.index_format == "csi" and rest == ["a.bam", "ref.fa"] and cli.split_own(["a.bam"])[0].index_format == "bai"
