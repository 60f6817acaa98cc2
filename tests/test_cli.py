"""cuteSV's command line and VCF header on this project's chain (cutesv_amd/cli.py, vcf.header_text).

CPU: the parser against what the reference's parseArgs returned for the same argument lists (golden/cli_args.json.gz), main's
refusals, and the header against the reference's Generation_VCF_header line for line (golden/vcf_header.json.gz).  GPU: main() on
the planted BAM - header + call_bam's body, the .sigs files of --write_old_sigs with and without --retain_work_dir, and flags that
reach the clustering."""
import os
import re
import time

import pytest

from cutesv_amd import call, cli, fasta, vcf
from cutesv_amd.columns import Params, TYPES
from helpers import load_json
import call_helpers

DATE_RE = r"##fileDate=\d{4}-\d\d-\d\d \d\d:\d\d:\d\d [0-6]-\S*"


# ------------------------------------------------------------------------------------------------ CPU: the parser
def test_parse_args_is_the_references_parser():
    cases = load_json("cli_args.json.gz")
    assert len(cases) >= 40
    seen = set()
    for case in cases:
        got = vars(cli.parse_args(case["argv"]))
        assert got == case["args"], case["argv"]
        assert all(type(got[k]) is type(v) for k, v in case["args"].items()), case["argv"]
        seen.update(x for x in case["argv"] if x.startswith("-") and not re.fullmatch(r"-\d+", x))
    # every spelling the parser knows was recorded
    known = {s for a in cli._parser()._actions for s in a.option_strings} - {"-h", "--help", "-v", "--version"}
    assert known == seen
    own, rest = cli.split_own(["a", "--tra_gt", "off", "b", "-t", "2", "--reads_table", "device", "c", "d"])
    assert (own.tra_gt, own.reads_table, rest) == ("off", "device", ["a", "b", "-t", "2", "c", "d"])
    assert vars(cli.parse_args(["a", "b", "c", "d", "--t", "3"]))["threads"] == 3          # (the reference's abbreviations still resolve)


def test_call_params_are_the_flags():
    a = cli.parse_args(["a", "b", "c", "d"])
    cp = cli.call_params(a)
    assert cp == call.CallParams(Params())                               # cuteSV's defaults are Params' and CallParams'
    a = cli.parse_args(["a", "b", "c", "d", "-s", "2", "-l", "50", "-L", "-1", "--genotype", "--gt_round", "9", "--max_cluster_bias_INS", "1", "--diff_ratio_merging_INS", "0.25",
                        "--max_cluster_bias_DEL", "2", "--diff_ratio_merging_DEL", "0.5", "--max_cluster_bias_INV", "3", "--max_cluster_bias_DUP", "4",
                        "--max_cluster_bias_TRA", "5", "--diff_ratio_filtering_TRA", "0.75", "--remain_reads_ratio", "0.5", "-q", "1", "-p", "-1", "-r", "7", "-sl", "8",
                        "-md", "9", "-mi", "10"])
    want = call.CallParams(Params(min_support=2, min_size=50, max_size=-1, genotype=True, gt_round=9, max_cluster_bias_INS=1, diff_ratio_merging_INS=0.25,
                                  max_cluster_bias_DEL=2, diff_ratio_merging_DEL=0.5, max_cluster_bias_INV=3, max_cluster_bias_DUP=4, max_cluster_bias_TRA=5,
                                  diff_ratio_filtering_TRA=0.75, remain_reads_ratio=0.5),
                           min_mapq=1, max_split_parts=-1, min_read_len=7, min_siglength=8, merge_del_threshold=9, merge_ins_threshold=10)
    assert cli.call_params(a) == want


def test_main_refuses_as_the_reference_does(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">c\nACGT\n")
    wd = tmp_path / "work"
    wd.mkdir()
    argv = ["in.bam", str(fa), str(tmp_path / "out.vcf"), str(wd)]
    with pytest.raises(ValueError, match="force calling"):
        cli.main(argv + ["-Ivcf", "x"])
    with pytest.raises(FileNotFoundError):
        cli.main(argv[:3] + [str(tmp_path / "nowhere")])
    with pytest.raises(FileNotFoundError):
        cli.main(["in.bam", str(tmp_path / "no.fa")] + argv[2:])
    (wd / "DEL.sigs").write_text("")
    with pytest.raises(FileExistsError):
        cli.main(argv)
    assert not (tmp_path / "out.vcf").exists()
    import cutesv_amd.__main__ as entry
    assert entry.main is cli.main


# ------------------------------------------------------------------------------------------------ CPU: the header
def test_header_is_the_references_line_for_line():
    cases = load_json("vcf_header.json.gz")
    assert [len(c["contigs"]) for c in cases] == [1, 25, 2] and cases[0]["sample"] == "NULL" and " " in cases[1]["sample"] and cases[2]["contigs"][0][1] == 0
    for c in cases:
        contigs = [tuple(x) for x in c["contigs"]]
        got = vcf.header_text(contigs, c["sample"], c["argv"])
        assert got.endswith("\n")
        lines, want = got.splitlines(), c["text"].splitlines()
        assert len(lines) == len(want) + 1
        differ = [k for k in range(len(want)) if lines[k] != want[k]]
        assert differ == [1, 2, len(want) - 1]
        assert lines[1] == "##source=cutesv_amd (cuteSV-2.1.4)" and want[1] == "##source=cuteSV-2.1.4"
        assert re.fullmatch(DATE_RE, lines[2]) and re.fullmatch(DATE_RE, want[2])
        assert lines[len(want) - 1] == '##CommandLine="cutesv_amd %s"' % " ".join(c["argv"])
        assert want[-1] == '##CommandLine="cuteSV %s"' % " ".join(c["argv"])
        assert lines[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + c["sample"]
        assert sum(1 for ln in lines if ln.startswith("##contig=")) == len(contigs)
    fixed = vcf.header_text([("c", 5)], "s", ["x"], now=time.struct_time((2026, 7, 12, 1, 2, 3, 6, 193, 0)))
    assert fixed.splitlines()[2].startswith("##fileDate=2026-07-12 01:02:03 0-")


# ------------------------------------------------------------------------------------------------ GPU: the command line end to end
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    path = str(d / "planted.bam")
    ref = call_helpers.write_planted_bam(path)
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return path, fa


def _masked(data):
    return re.sub(rb"(?m)^##fileDate=.*$", b"##fileDate=", data)


def _expected(path, fa, argv, sample, cp, **kw):
    body, _ = call.call_bam(path, fasta.Reference(fa), cp, as_bytes=True, **kw)
    return _masked(vcf.header_text(call_helpers.CONTIGS, sample, argv).encode()) + body, body


@pytest.mark.gpu
def test_gpu_main_writes_a_vcf_file_and_the_sigs_files(planted, tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("CUTESV_AMD_TRA_GT", raising=False)
    path, fa = planted
    out, wd = str(tmp_path / "out.vcf"), str(tmp_path / "work")
    os.mkdir(wd)
    argv = [path, fa, out, wd, "-s", "1", "--genotype", "--report_readid", "-S", "HG002", "--write_old_sigs", "--retain_work_dir"]
    assert cli.main(argv) == 0
    cp = call.CallParams(Params(min_support=1, genotype=True))
    want, body = _expected(path, fa, argv, "HG002", cp, report_readid=True, tra_gt="alignments")
    with open(out, "rb") as f:
        got = f.read()
    assert _masked(got) == want
    assert body.count(b"\n") >= 5 and b"RNAMES=" in body and re.search(DATE_RE.encode(), got)
    assert got.split(b"\n")[len(call_helpers.CONTIGS) + 3].startswith(b"##ALT=")
    assert sorted(os.listdir(wd)) == sorted(t + ".sigs" for t in TYPES)
    kept = {t: open(os.path.join(wd, t + ".sigs"), "rb").read() for t in TYPES}
    assert kept["INS"].count(b"\n") >= 18 and kept["DEL"].startswith(b"DEL\tchrA\t")
    assert "records" in capsys.readouterr().err
    # a second run into the same work directory is refused, as in the reference
    with pytest.raises(FileExistsError):
        cli.main(argv)
    # without --retain_work_dir the files of this run are removed again
    wd2 = str(tmp_path / "work2")
    os.mkdir(wd2)
    out2 = str(tmp_path / "out2.vcf")
    argv2 = [path, fa, out2, wd2] + argv[4:-1]
    assert cli.main(argv2) == 0
    assert os.listdir(wd2) == []
    with open(out2, "rb") as f:
        assert _masked(f.read()) == _masked(vcf.header_text(call_helpers.CONTIGS, "HG002", argv2).encode()) + body
    # flags that reach the clustering and the filters change the body exactly as call_bam with those Params does
    out3 = str(tmp_path / "out3.vcf")
    argv3 = [path, fa, out3, wd2, "-s", "1", "--max_cluster_bias_DEL", "1", "-l", "50"]
    assert cli.main(argv3) == 0
    want3, body3 = _expected(path, fa, argv3, "NULL", call.CallParams(Params(min_support=1, max_cluster_bias_DEL=1, min_size=50)))
    with open(out3, "rb") as f:
        assert _masked(f.read()) == want3
    assert os.listdir(wd2) == []
    # ... and a filter that does bite on this file: the 200-base DEL and the 150-base INS go
    argv4 = [path, fa, out3, wd2, "-s", "1", "--min_size", "250"]
    assert cli.main(argv4) == 0
    want4, body4 = _expected(path, fa, argv4, "NULL", call.CallParams(Params(min_support=1, min_size=250)))
    with open(out3, "rb") as f:
        assert _masked(f.read()) == want4
    assert 0 < body4.count(b"\n") < body3.count(b"\n") and b"SVTYPE=DEL" in body3 and b"SVTYPE=DEL" not in body4
