"""call_bam's host side without a GPU and without the library: the options resolver - defaults, every refusal with
the text it had while the checks were inlined in call_bam, and which of two refusals fires first; the option declaration the two command
lines share; the reference both of them close; the reader session on a fake reader and a fake context."""
import argparse

import numpy as np
import pytest

from cutesv_amd import bam, bed, call, cli, engine, fasta
from cutesv_amd.columns import Params

# the refusals of call_bam in the order in which they fire, texts copied from the body they were inlined in
M_INDEX_FORMAT = "index_format must be 'bai' or 'csi', not 'bogus'"
M_REF_ROUTE = "ref_route must be 'host' or 'device', not 'bogus'"
M_TASK_CUT = "task_cut must be None, 'uniform' or 'index', not 'bogus'"
M_NO_INDEX = "task_cut='index' needs a BAM index (.bai): this reader has none"
M_READS_TABLE = "reads_table must be 'host' or 'device', not 'bogus'"
M_FRAME = "frame must be 'host' or 'device', not 'bogus'"
M_FRAME_INFLATE = "frame='device' needs the device inflate: inflate='host' cannot be combined with it"
M_INFLATE = "inflate must be 'host' or 'device', not 'bogus'"
M_TRA = ("call_bam genotypes TRA calls with CUTESV_AMD_TRA_GT=alignments (from every alignment, as the reference does) or "
         "CUTESV_AMD_TRA_GT=reads_table, or leaves them with CUTESV_AMD_TRA_GT=off; 'bam' is not available here "
         "(the pysam-based mode needs resolve.phase3 with bam=)")
M_CUT_THREADS = "cut_threads must be a positive integer, not 0"
M_NOT_FOUND = "task_cut='index' needs a BAM index (.bai): none was found for in.bam"


class _Stub:
    """what the resolver reads of an open reader"""
    references, has_index = ("chrA",), False


@pytest.fixture
def bad_bed(tmp_path):
    path = tmp_path / "bad.bed"
    path.write_text("chrA\t10\n")
    return str(path), "%s:1: a BED line needs three tab-separated fields (chrom, start, end), found 2" % path


def _refused(message, bam_arg="in.bam", index=None, params=None, **kw):
    with pytest.raises(ValueError) as e:
        call.resolve_options(bam_arg, index, params or Params.ont(), **kw)
    assert str(e.value) == message


# ------------------------------------------------------------------------------------------------ defaults
def test_every_option_left_out_takes_its_default():
    o = call.resolve_options("in.bam", None, Params.ont())
    assert (o.reads_table, o.frame, o.inflate, o.gates) == (call.DEFAULT_READS_TABLE, call.DEFAULT_FRAME, call.DEFAULT_INFLATE, call.DEFAULT_GATES)
    assert o.ref_route is None and o.regions is None and o.mode == "off" and o.task_cut is None and o.cut_threads == 16
    assert o.index_format == "bai" and o.build_index is False and o.reads_dev is False
    assert isinstance(o.cp, call.CallParams) and o.cp.resolve == Params.ont() and o.p == Params.ont() and o.p.genotype_tra is False
    with pytest.raises(Exception):                                # frozen
        o.frame = "device"
    cp = call.CallParams(Params.ont(min_support=3), min_mapq=7)
    assert call.resolve_options("in.bam", None, cp).cp is cp


def test_the_defaults_are_read_at_the_call(monkeypatch):
    monkeypatch.setattr(call, "DEFAULT_INFLATE", "device")
    assert call.resolve_options("in.bam", None, Params.ont()).inflate == "device"
    monkeypatch.setattr(call, "DEFAULT_READS_TABLE", "device")
    monkeypatch.setattr(call, "DEFAULT_FRAME", "device")
    monkeypatch.setattr(call, "DEFAULT_GATES", "host")
    o = call.resolve_options("in.bam", None, Params.ont())
    assert (o.reads_table, o.frame, o.gates) == ("device", "device", "host")


def test_device_framing_takes_the_device_inflate():
    o = call.resolve_options("in.bam", None, Params.ont(), frame="device")
    assert (o.frame, o.inflate) == ("device", "device")
    assert call.resolve_options("in.bam", None, Params.ont(), frame="device", inflate="device").inflate == "device"
    assert call.resolve_options("in.bam", None, Params.ont(), frame="host", inflate="device").frame == "host"


def test_a_bed_takes_the_device_gates(tmp_path):
    regions = bed.Regions.from_intervals({"chrA": [(100, 200)]})
    o = call.resolve_options("in.bam", None, Params.ont(), include_bed=regions)
    assert o.gates == "device" and o.regions is regions
    path = tmp_path / "panel.bed"
    path.write_text("chrA\t100\t200\nchrB\t5000\t6000\n")
    o = call.resolve_options("in.bam", None, Params.ont(), include_bed=str(path))
    assert o.gates == "device" and isinstance(o.regions, bed.Regions)
    assert {c: a.tolist() for c, a in o.regions.by_chrom.items()} == {"chrA": [[-900, 1200]], "chrB": [[4000, 7000]]}
    assert call.resolve_options("in.bam", None, Params.ont(), include_bed=regions, gates="host").gates == "host"


def test_gates_are_not_checked_here():
    assert call.resolve_options("in.bam", None, Params.ont(), gates="bogus").gates == "bogus"       # (extract.task_to_pool refuses it at the first task)


def test_tra_mode(monkeypatch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "alignments")
    for tra_gt in (None, "alignments", "reads_table", "bam"):
        o = call.resolve_options("in.bam", None, Params.ont(genotype=False), tra_gt=tra_gt)
        assert o.mode == "off" and o.p.genotype_tra is False
    assert call.resolve_options("in.bam", None, Params.ont(genotype=True)).mode == "alignments"
    o = call.resolve_options("in.bam", None, Params.ont(genotype=True), tra_gt="reads_table", reads_table="device")
    assert o.mode == "reads_table" and o.p.genotype_tra is True and o.cp.resolve.genotype_tra is False and o.reads_dev is True
    assert call.resolve_options("in.bam", None, Params.ont(genotype=False), reads_table="device").reads_dev is False
    monkeypatch.delenv("CUTESV_AMD_TRA_GT")
    _refused(M_TRA, params=Params.ont(genotype=True))


def test_index_build_is_for_a_path():
    assert call.resolve_options("in.bam", "build", Params.ont(), task_cut="index", index_format="csi").build_index is True
    assert call.resolve_options(_Stub(), "build", Params.ont()).build_index is False
    assert call.resolve_options("in.bam", "in.bam.bai", Params.ont(), task_cut="index").build_index is False


# ------------------------------------------------------------------------------------------------ refusals and their order
def test_every_refusal_keeps_its_text(bad_bed):
    _refused(M_INDEX_FORMAT, index_format="bogus")
    _refused(M_REF_ROUTE, ref_route="bogus")
    _refused(M_TASK_CUT, task_cut="bogus")
    _refused(M_NO_INDEX, bam_arg=_Stub(), task_cut="index")
    _refused(M_NO_INDEX, index=False, task_cut="index")
    _refused(M_READS_TABLE, reads_table="bogus")
    _refused(M_FRAME, frame="bogus")
    _refused(M_FRAME_INFLATE, frame="device", inflate="host")
    _refused(M_INFLATE, inflate="bogus")
    _refused(bad_bed[1], include_bed=bad_bed[0])
    with pytest.raises(FileNotFoundError):
        call.resolve_options("in.bam", None, Params.ont(), include_bed="no_such.bed")
    _refused(M_TRA, params=Params.ont(genotype=True), tra_gt="bam")
    # the one check that moved here from behind the pool reset: only the index cut looks at cut_threads
    _refused(M_CUT_THREADS, task_cut="index", cut_threads=0)
    _refused("cut_threads must be a positive integer, not 2.0", task_cut="index", cut_threads=2.0)
    assert call.resolve_options("in.bam", None, Params.ont(), task_cut="uniform", cut_threads=0).cut_threads == 0
    assert call.resolve_options("in.bam", None, Params.ont(), task_cut="index", cut_threads=np.int64(3)).cut_threads == 3


def test_of_two_refusals_the_earlier_one_fires(bad_bed):
    """every neighbouring pair of the order.  Two pairs cannot be wrong both ways in one call - a task_cut that is no known value is not
    'index', an inflate that is no known value is not 'host' - so each of them is bracketed from both sides: 2 before 4 and 3 before 5, 6 before 8
    and 7 before 9."""
    gt = Params.ont(genotype=True)
    _refused(M_INDEX_FORMAT, index_format="bogus", ref_route="bogus")                                    # 1 before 2
    _refused(M_REF_ROUTE, ref_route="bogus", task_cut="bogus")                                           # 2 before 3
    _refused(M_REF_ROUTE, index=False, ref_route="bogus", task_cut="index")                              # 2 before 4
    _refused(M_TASK_CUT, task_cut="bogus", reads_table="bogus")                                          # 3 before 5
    _refused(M_NO_INDEX, index=False, task_cut="index", reads_table="bogus")                             # 4 before 5
    _refused(M_NO_INDEX, bam_arg=_Stub(), task_cut="index", reads_table="bogus")
    _refused(M_READS_TABLE, reads_table="bogus", frame="bogus")                                          # 5 before 6
    _refused(M_FRAME, frame="bogus", inflate="host")                                                     # 6 before 7 (the cross rule needs a known frame)
    _refused(M_FRAME, frame="bogus", inflate="bogus")                                                    # 6 before 8
    _refused(M_FRAME_INFLATE, frame="device", inflate="host", include_bed=bad_bed[0])                    # 7 before 9
    _refused(M_INFLATE, inflate="bogus", include_bed=bad_bed[0])                                         # 8 before 9
    _refused(bad_bed[1], params=gt, include_bed=bad_bed[0], tra_gt="bam")                                # 9 before 10
    _refused(M_TRA, params=gt, tra_gt="bam", task_cut="index", cut_threads=0)                            # 10 before the cut_threads check
    _refused(M_INDEX_FORMAT, index_format="bogus", task_cut="index", cut_threads=0)


def test_call_bam_refuses_through_the_resolver_before_it_opens_anything():
    with pytest.raises(ValueError) as e:
        call.call_bam("no_such.bam", {}, Params.ont(), frame="device", inflate="host")
    assert str(e.value) == M_FRAME_INFLATE
    with pytest.raises(ValueError) as e:
        call.call_bam("no_such.bam", {}, Params.ont(), task_cut="index", cut_threads=0)
    assert str(e.value) == M_CUT_THREADS


# ------------------------------------------------------------------------------------------------ the two command lines
SHARED = dict(reads_table=("host", "device"), tra_gt=call.TRA_GT_MODES, inflate=("host", "device"), frame=("host", "device"), ref_route=("host", "device"))


@pytest.fixture
def stub_call(monkeypatch):
    """call.call_bam replaced by a recorder of its keywords (or by what `fail` holds), fasta.open_reference by one of close()"""
    class Ref:
        closed = 0

        def close(self):
            Ref.closed += 1

    seen, fail = [], []

    def stub(*a, **k):
        seen.append((a, k))
        if fail:
            raise fail[0]
        return b"", np.zeros(5, np.int64)
    monkeypatch.setattr(call, "call_bam", stub)
    monkeypatch.setattr(fasta, "open_reference", lambda path, **kw: Ref())
    return seen, fail, Ref


def _cli_argv(monkeypatch, tmp_path):
    """what cli.main needs around the call: a reference file, a work directory and a reader it can open without the library"""
    class Reader:
        references, lengths, has_index = ("chrA",), (1000,), True

        def __init__(self, path, threads=None):
            pass

        def close(self):
            pass
    monkeypatch.setattr(bam, "BamFile", Reader)
    (tmp_path / "ref.fa").write_text(">chrA\nACGT\n")
    (tmp_path / "work").mkdir(exist_ok=True)
    return ["in.bam", str(tmp_path / "ref.fa"), str(tmp_path / "out.vcf"), str(tmp_path / "work")]


def test_one_declaration_feeds_both_parsers(monkeypatch, tmp_path, stub_call):
    ap = argparse.ArgumentParser()
    call.add_route_options(ap)
    declared = {a.dest: tuple(a.choices) for a in ap._actions if a.dest in SHARED}
    assert declared == {k: tuple(v) for k, v in SHARED.items()}
    own = {a.dest: tuple(a.choices) for a in cli._own_parser()._actions if a.dest in SHARED}
    assert own == declared and all(a.default is None for a in cli._own_parser()._actions if a.dest in SHARED)
    seen = stub_call[0]
    out = str(tmp_path / "o.vcf")
    for name, choices in SHARED.items():
        for choice in choices:
            ns, rest = cli.split_own(["a", "--" + name, choice, "b"])
            assert getattr(ns, name) == choice and rest == ["a", "b"]
            assert call.main(["a.bam", "ref.fa", "-o", out, "--" + name, choice]) == 0
            assert seen[-1][1][name] == choice
        with pytest.raises(SystemExit):
            cli.split_own(["--" + name, "bogus"])
        with pytest.raises(SystemExit):
            call.main(["a.bam", "ref.fa", "-o", out, "--" + name, "bogus"])
        assert getattr(cli.split_own([])[0], name) is None
    assert cli.split_own(["--infl", "device"])[1] == ["--infl", "device"]              # (no abbreviations: they are cuteSV's parser's to refuse)


def test_a_command_line_genotypes_tra_from_alignments_unless_told_otherwise(monkeypatch, tmp_path, stub_call):
    monkeypatch.delenv("CUTESV_AMD_TRA_GT", raising=False)
    assert call.command_line_tra_gt(None, True) == "alignments" and call.command_line_tra_gt(None, False) is None
    assert call.command_line_tra_gt("off", True) == "off"
    seen = stub_call[0]
    argv = _cli_argv(monkeypatch, tmp_path)
    out = str(tmp_path / "o.vcf")
    assert call.main(["a.bam", "ref.fa", "-o", out, "--genotype"]) == 0 and cli.main(argv + ["--genotype"]) == 0
    assert [k["tra_gt"] for _, k in seen] == ["alignments", "alignments"]
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "reads_table")
    assert call.command_line_tra_gt(None, True) is None
    assert call.main(["a.bam", "ref.fa", "-o", out, "--genotype"]) == 0 and cli.main(argv + ["--genotype"]) == 0
    assert [k["tra_gt"] for _, k in seen[2:]] == [None, None]


def test_both_command_lines_close_their_reference(monkeypatch, tmp_path, stub_call):
    seen, fail, ref = stub_call
    argv = _cli_argv(monkeypatch, tmp_path)
    assert call.main(["a.bam", "ref.fa", "-o", str(tmp_path / "o.vcf")]) == 0
    assert ref.closed == 1 and isinstance(seen[-1][0][1], ref)
    assert cli.main(argv) == 0
    assert ref.closed == 2 and isinstance(seen[-1][0][1], ref)
    fail.append(RuntimeError("the call failed"))
    with pytest.raises(RuntimeError, match="the call failed"):
        call.main(["a.bam", "ref.fa", "-o", str(tmp_path / "o.vcf")])
    assert ref.closed == 3
    with pytest.raises(RuntimeError, match="the call failed"):
        cli.main(argv)
    assert ref.closed == 4


# ------------------------------------------------------------------------------------------------ the reader session
class FakeReader:
    """bam.BamFile as the session uses it; every call goes into `log`"""
    log = None

    def __init__(self, path, threads=None, index=None, has_index=False, inflate=None, frame=None, refuse=()):
        self.path, self.has_index, self.inflate, self.frame, self.refuse = path, has_index, inflate, frame, refuse
        self.log.append(("open", path, index))

    def set_inflate(self, inflate):
        self.log.append(("set_inflate", inflate))
        previous, self.inflate = self.inflate, inflate
        return previous

    def set_frame(self, frame):
        self.log.append(("set_frame", frame))
        if "set_frame" in self.refuse:
            raise bam.BamError("the frame route cannot be set")
        self.frame = self.inflate if frame == "device" else None

    def build_index(self, format="bai"):
        self.log.append(("build_index", format))
        if "build_index" in self.refuse:
            raise bam.BamError("a record is out of order")
        self.has_index = True

    def close(self):
        self.log.append(("close", "reader"))


class FakeContext:
    def __init__(self, log):
        self.log = log
        log.append(("open", "context"))

    def close(self):
        self.log.append(("close", "context"))


@pytest.fixture
def log(monkeypatch):
    log = []
    monkeypatch.setattr(FakeReader, "log", log)
    monkeypatch.setattr(bam, "BamFile", FakeReader)
    monkeypatch.setattr(engine, "Context", lambda device: FakeContext(log))
    return log


def _opts(index=None, **kw):
    return call.resolve_options("in.bam", index, Params.ont(), **kw)


def test_the_session_closes_its_reader_before_its_context(log):
    with call._session("in.bam", None, _opts(), 3, None, None, None) as (bf, ctx, laps):
        assert isinstance(bf, FakeReader) and isinstance(ctx, FakeContext)
        assert log == [("open", "in.bam", None), ("open", "context"), ("set_inflate", None), ("set_frame", "host")]
        laps.lap("ms_tasks")                                      # (costs nothing without a dict)
        del log[:]
    assert log == [("close", "reader"), ("close", "context")]


def test_the_session_sets_the_device_routes_on_its_context(log):
    with call._session("in.bam", None, _opts(frame="device"), None, None, None, None) as (bf, ctx, _):
        assert log[2:] == [("set_inflate", ctx), ("set_frame", "device")]


def test_a_context_that_cannot_be_created_closes_the_reader_the_session_opened(log, monkeypatch):
    def no_device(device):
        raise RuntimeError("no device")
    monkeypatch.setattr(engine, "Context", no_device)
    with pytest.raises(RuntimeError, match="no device"):
        with call._session("in.bam", None, _opts(), None, None, None, None):
            pass
    assert log == [("open", "in.bam", None), ("close", "reader")]


def test_a_refused_frame_route_puts_a_borrowed_readers_routes_back(log):
    device = FakeContext(log)
    reader = FakeReader("in.bam", inflate=device, frame=device, refuse=("set_frame",))
    ctx = FakeContext(log)
    del log[:]
    with pytest.raises(bam.BamError):
        with call._session(reader, ctx, _opts(), None, None, None, None):
            pass
    assert log == [("set_inflate", None), ("set_frame", "host"), ("set_inflate", device), ("set_frame", "device")]


def test_a_borrowed_reader_and_a_borrowed_context_are_never_closed(log):
    reader, ctx = FakeReader("in.bam", inflate="before"), FakeContext(log)
    del log[:]
    with call._session(reader, ctx, _opts(inflate="device"), None, None, None, None) as (bf, c, _):
        assert bf is reader and c is ctx and reader.inflate is ctx
    assert log == [("set_inflate", ctx), ("set_frame", "host"), ("set_inflate", "before")] and reader.inflate == "before"
    with pytest.raises(KeyError):
        with call._session(reader, ctx, _opts(), None, None, None, None):
            raise KeyError("chrZ")
    assert ("close", "reader") not in log and ("close", "context") not in log and log[-1] == ("set_inflate", "before")


def test_the_session_builds_the_index_on_the_calls_routes_and_laps_it_first(log):
    timings = {}
    with call._session("in.bam", None, _opts(index="build", task_cut="index", index_format="csi", inflate="device"), None, "build", timings, None) as (bf, ctx, laps):
        assert log == [("open", "in.bam", None), ("open", "context"), ("set_inflate", ctx), ("set_frame", "host"), ("build_index", "csi")]
        laps.lap("ms_tasks")
    assert list(timings) == ["ms_index", "ms_tasks"] and log[-2:] == [("close", "reader"), ("close", "context")]


def test_a_failed_index_build_releases_reader_and_context(log, monkeypatch):
    class Unsorted(FakeReader):
        def __init__(self, path, **kw):
            FakeReader.__init__(self, path, refuse=("build_index",), **kw)
    monkeypatch.setattr(bam, "BamFile", Unsorted)
    with pytest.raises(bam.BamError, match="out of order"):
        with call._session("in.bam", None, _opts(index="build"), None, "build", None, None):
            pass
    assert log[-3:] == [("build_index", "bai"), ("close", "reader"), ("close", "context")]


def test_the_index_cut_without_an_index_is_refused_where_the_reader_is_known(log):
    with pytest.raises(ValueError) as e:
        with call._session("in.bam", None, _opts(task_cut="index"), None, None, None, None):
            pass
    assert str(e.value) == M_NOT_FOUND
    assert log == [("open", "in.bam", None), ("open", "context"), ("close", "reader"), ("close", "context")]


def test_the_sums_over_the_tasks():
    timings, read_stats = {}, {}
    laps = call._Laps(timings, read_stats)
    for n in (5, 7):
        laps.add_task(dict(ms_inflate=1.5, ms_frame=0.25, compressed_bytes=100), dict(n_records=n))
    laps.lap("ms_tasks")
    assert list(timings) == ["ms_inflate", "ms_frame", "ms_tasks"] and (timings["ms_inflate"], timings["ms_frame"]) == (3.0, 0.5) and timings["ms_tasks"] >= 0
    assert read_stats == dict(compressed_bytes=200, n_records=12, task_records=[5, 7])
    call._Laps(None, None).add_task({}, {})                       # (nothing is read of either without a dict)
