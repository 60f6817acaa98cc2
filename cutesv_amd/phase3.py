"""Phase 3 of cuteSV on its own work directory, in one call: `resolve.phase3` from the command line.

    python -m cutesv_amd.phase3 WORK_DIR [--preset ont|hifi|clr] [--genotype] [--fasta REF.fa] [--bam BAM] -o OUT
    python -m cutesv_amd.phase3 WORK_DIR ... --digest -o OUT.json

WORK_DIR holds what cuteSV's signature step leaves there (main script :817-857): `<TYPE>.pickle`, `reads.pickle` and
`sigindex.pickle`.  The clustering of every chromosome and type runs as one batch per GPU; OUT receives the VCF body the
reference's generate_output would write for those calls (vcf.emit_stage; needs --fasta), or with --digest a JSON object
{"TYPE:chr": [rows, sha256 of the rows]} - the read names of a row sorted, so that it does not depend on their order.
TRA genotyping follows CUTESV_AMD_TRA_GT (bam - needs --bam -, reads_table, off); without --bam it is off.
"""
import argparse
import hashlib
import json
import os
import pickle
import sys

from . import resolve
from .columns import Params

_READS_FIELD = {"DEL": 12, "INS": 12, "DUP": 10, "INV": 11, "TRA": 11}     # the comma-joined read names of a row


def digests(results):
    """{chr: rows} -> {"TYPE:chr": [n, sha256 hex]}: the rows of each (type, chromosome), tab-joined, read names sorted"""
    per = {}
    for ch, rows in results.items():
        for r in rows:
            t = r[1] if r[1] in ("DEL", "INS", "DUP", "INV") else "TRA"
            row = list(r)
            k = _READS_FIELD[t]
            row[k] = ",".join(sorted(row[k].split(",")))
            per.setdefault("%s:%s" % (t, ch), []).append("\t".join(row))
    return {k: [len(v), hashlib.sha256("\n".join(v).encode()).hexdigest()] for k, v in per.items()}


def main(argv=None, ctx=None):
    ap = argparse.ArgumentParser(prog="python -m cutesv_amd.phase3", description=__doc__.split("\n\n")[0])
    ap.add_argument("work_dir")
    ap.add_argument("--preset", choices=["ont", "hifi", "clr"], default=None, help="cuteSV's recommended clustering flags")
    ap.add_argument("--genotype", action="store_true")
    ap.add_argument("--min-support", type=int, default=None)
    ap.add_argument("--fasta", default=None, help="reference FASTA (the REF bases of the VCF body)")
    ap.add_argument("--bam", default=None, help="the BAM, to genotype TRA calls from it (CUTESV_AMD_TRA_GT=bam)")
    ap.add_argument("--threads", type=int, default=None, help="host threads of the walk (default: min(16, CPUs))")
    ap.add_argument("--digest", action="store_true", help="write per-(type, chromosome) digests of the rows as JSON instead")
    ap.add_argument("-o", "--out", required=True)
    a = ap.parse_args(argv)
    if not a.digest and not a.fasta:
        ap.error("the VCF body needs --fasta (or ask for --digest)")
    kw = dict(genotype=a.genotype)
    if a.min_support is not None:
        kw["min_support"] = a.min_support
    p = getattr(Params, a.preset)(**kw) if a.preset else Params(**kw)
    wd = a.work_dir if a.work_dir.endswith("/") else a.work_dir + "/"
    with open(wd + "sigindex.pickle", "rb") as f:
        sigs_index = pickle.load(f)
    if a.genotype and a.bam is None and os.environ.get("CUTESV_AMD_TRA_GT", "bam") == "bam":
        os.environ["CUTESV_AMD_TRA_GT"] = "off"
    results = resolve.phase3(wd, sigs_index, p, bam=a.bam, threads=a.threads, lazy=not a.digest, ctx=ctx)
    if a.digest:
        with open(a.out, "w") as f:
            json.dump(digests(results), f, indent=0, sort_keys=True)
        return 0
    from . import fasta, vcf
    text, _ = vcf.emit_stage(results, fasta.open_reference(a.fasta), min_size=p.min_size, max_size=p.max_size, genotype=p.genotype,
                             as_bytes=True)
    with open(a.out, "wb") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
