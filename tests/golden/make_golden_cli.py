#!/usr/bin/env python3
"""Golden vectors of the reference's command line and VCF header (src/cuteSV/cuteSV_Description.py), produced by running it here.

    python tests/golden/make_golden_cli.py         # needs the reference checkout (read-only mount)

The module is imported at generation time only, the way make_golden_main.py imports the main script.  Nothing of the reference is
copied: the outputs are data - argument lists we write and what the reference's two functions return for them.

Outputs
    vcf_header.json.gz   Generation_VCF_header (:265-305) for three inputs: one contig with the default sample, 25 contigs with a
                         sample name that contains a blank, a contig of length 0: [{contigs, sample, argv, text}]
    cli_args.json.gz     vars(parseArgs(argv)) (:53-263) for the bare positionals, for every flag set once to a non-default value
                         under each of its spellings, and for one argv with everything set: [{argv, args}]
"""
import gzip
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

POSITIONALS = ["in.bam", "ref.fa", "out.vcf", "work/"]
# (spellings, a non-default value; None: a switch)
FLAGS = [
    (("-t", "--threads"), "3"), (("-b", "--batches"), "250000"), (("-S", "--sample"), "HG 002"), (("--retain_work_dir",), None),
    (("--write_old_sigs",), None), (("--report_readid",), None), (("--ignore_sequence",), None), (("-p", "--max_split_parts"), "-1"),
    (("-q", "--min_mapq"), "7"), (("-r", "--min_read_len"), "1234"), (("-md", "--merge_del_threshold"), "500"), (("-mi", "--merge_ins_threshold"), "501"),
    (("-include_bed",), "regions.bed"), (("-s", "--min_support"), "2"), (("-l", "--min_size"), "50"), (("-L", "--max_size"), "-1"),
    (("-sl", "--min_siglength"), "11"), (("--genotype",), None), (("--gt_round",), "99"), (("--read_range",), "2000"), (("-Ivcf",), "given.vcf"),
    (("--max_cluster_bias_INS",), "1000"), (("--diff_ratio_merging_INS",), "0.9"), (("--max_cluster_bias_DEL",), "1001"), (("--diff_ratio_merging_DEL",), "0.45"),
    (("--max_cluster_bias_INV",), "501"), (("--max_cluster_bias_DUP",), "502"), (("--max_cluster_bias_TRA",), "51"), (("--diff_ratio_filtering_TRA",), "0.65"),
    (("--remain_reads_ratio",), "0.75"),
]


def main():
    sys.path.insert(0, os.path.join(REF, "src", "cuteSV"))
    import cuteSV_Description as desc
    argvs = [list(POSITIONALS)]
    everything = list(POSITIONALS)
    for spellings, value in FLAGS:
        for sp in spellings:
            argvs.append(POSITIONALS + [sp] + ([] if value is None else [value]))
        everything += [spellings[-1]] + ([] if value is None else [value])
    argvs.append(everything)
    argvs.append(POSITIONALS[:2] + ["-s", "3", "--genotype"] + POSITIONALS[2:])        # (flags between the positionals)
    cases = [dict(argv=a, args=vars(desc.parseArgs(a))) for a in argvs]
    with gzip.open(os.path.join(HERE, "cli_args.json.gz"), "wt") as f:
        json.dump(cases, f)
    print("cli_args.json.gz: %d argument lists" % len(cases))

    headers = []
    for contigs, sample, argv in (([["chr1", 248956422]], "NULL", list(POSITIONALS)),
                                  ([["chr%d" % i, 1000 * i + 7] for i in range(1, 23)] + [["chrX", 156040895], ["chrY", 57227415], ["chrM", 16569]], "HG 002",
                                   POSITIONALS + ["-S", "HG 002", "--genotype", "-s", "3"]),
                                  ([["empty", 0], ["GL000207.1", 4262]], "s", POSITIONALS + ["-l", "50"])):
        buf = io.StringIO()
        desc.Generation_VCF_header(buf, contigs, sample, argv)
        headers.append(dict(contigs=contigs, sample=sample, argv=argv, text=buf.getvalue()))
    with gzip.open(os.path.join(HERE, "vcf_header.json.gz"), "wt") as f:
        json.dump(headers, f)
    print("vcf_header.json.gz: %d headers" % len(headers))


if __name__ == "__main__":
    main()
