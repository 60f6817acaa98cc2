#!/usr/bin/env python3
"""Golden vectors of the reference's legacy text signature files (--write_old_sigs), produced by running its main script here.

    python tests/golden/make_golden_sigs.py        # needs the reference checkout (read-only mount)

The main script is imported at generation time only, through make_golden_main.load_main.  Nothing of the reference is copied:
the outputs are data - the candidates we synthesise and the files the reference's function writes for them.

Output
    old_sigs.json.gz   for every case of rebuild_order.json.gz, and for one crafted case, the five texts DEL.sigs .. TRA.sigs that
                       process_process_sigs_type((type, dir, pids, True)) (main script :750-808) writes on the case's per-worker
                       pickles: [{name, sigs: {TYPE: text}}]; the crafted case also carries its `files` and the sorted lists
                       `out`, in the layout of rebuild_order.json.gz.  What is crafted: an INS position at x.5, an exact INS
                       duplicate, an INS tie group (same position, length and read, different bases), all four TRA types to two
                       mate contigs, both INV strands, a contig without rows of some types.
"""
import gzip
import json
import os
import pickle
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

SVTYPES = ("DEL", "INS", "DUP", "INV", "TRA")


def crafted_files():
    """two workers' candidate batches, in the layout rebuild_case makes"""
    ins = [(100.5, 40, "readB", "ACGT" * 10, "INS", "chr2"), (100, 40, "readB", "ACGT" * 10, "INS", "chr2"),       # x.5 and x: both stay
           (250, 12, "readA", "TTTTGGGGCCCC", "INS", "chr1"), (250, 12, "readA", "TTTTGGGGCCCC", "INS", "chr1"),    # an exact duplicate
           (300, 8, "tie", "GGGGGGGG", "INS", "chr1"), (300, 8, "tie", "AAAAAAAA", "INS", "chr1"), (300, 8, "tie", "CCCCCCCC", "INS", "chr1"),   # a tie group
           (7, 1, "r/1", "N", "INS", "chr10")]
    dele = [(1000, 35, "readA", "DEL", "chr1"), (1000, 35, "readA", "DEL", "chr1"), (999, 400, "readB", "DEL", "chr1"), (0, 30, "r/1", "DEL", "chr10")]
    dup = [(500, 1500, "readA", "DUP", "chr2"), (500, 1400, "readB", "DUP", "chr2")]
    inv = [("++", 2000, 2900, "readA", "INV", "chr1"), ("--", 1500, 2600, "readA", "INV", "chr1"), ("--", 1500, 2600, "readB", "INV", "chr1"),
           ("++", 10, 900, "r/1", "INV", "chr2")]
    tra = [(k, 4000 + 10 * i, mate, 77 + i, "read%s" % k, "TRA", "chr1") for i, (k, mate) in
           enumerate([("A", "chr2"), ("B", "chr2"), ("C", "chr2"), ("D", "chr2"), ("A", "chr10"), ("B", "chr10"), ("C", "chr10"), ("D", "chr10")])]
    tra += [("A", 4000, "chr2", 77, "readA", "TRA", "chr1"), ("D", 5, "chr1", 6, "r/1", "TRA", "chr2")]
    per = dict(DEL=dele, INS=ins, DUP=dup, INV=inv, TRA=tra)
    files = [{t: [] for t in SVTYPES + ("reads",)}, {t: [] for t in SVTYPES + ("reads",)}]       # (no reads table: reads.sigs is not recorded)
    for t, lst in per.items():
        files[0][t].append(lst[1::2])
        files[1][t].append(lst[0::2][::-1])
        files[1][t].append([])
    return files


def run_sigs(main, files, want_out=False):
    """-> ({TYPE: text of TYPE.sigs}, the sorted per-chromosome lists when want_out)"""
    pids = [1000 + i for i in range(len(files))]
    sigs, out = {}, {}
    with tempfile.TemporaryDirectory() as d:
        d = d + "/"
        os.mkdir(d + "signatures")
        for pid, f in zip(pids, files):
            for t in SVTYPES:
                with open("%ssignatures/%s%s.pickle" % (d, pid, t), "wb") as fh:
                    for b in f[t]:
                        pickle.dump([tuple(x) for x in b], fh)
        for t in SVTYPES:
            _, index, _ = main.process_process_sigs_type((t, d, pids, True))
            with open("%s%s.sigs" % (d, t)) as fh:
                sigs[t] = fh.read()
            if want_out:
                per_chr = []
                with open("%s%s.pickle" % (d, t), "rb") as fh:
                    for ch, off in sorted(index.items(), key=lambda kv: kv[1]):
                        fh.seek(off)
                        per_chr.append([ch, [list(x) for x in pickle.load(fh)]])
                out[t] = per_chr
    return sigs, out


def main_():
    from make_golden_main import load_main
    main = load_main()
    with gzip.open(os.path.join(HERE, "rebuild_order.json.gz"), "rt") as f:
        cases = json.load(f)
    recorded = []
    for case in cases:
        sigs, _ = run_sigs(main, case["files"])
        recorded.append(dict(name=case["name"], sigs=sigs))
    files = crafted_files()
    sigs, out = run_sigs(main, files, want_out=True)
    recorded.append(dict(name="crafted", files=[{t: [[list(x) for x in b] for b in bs] for t, bs in f.items()} for f in files], out=out, sigs=sigs))
    with gzip.open(os.path.join(HERE, "old_sigs.json.gz"), "wt") as f:
        json.dump(recorded, f)
    print("old_sigs.json.gz: %d cases, %d lines" % (len(recorded), sum(s.count("\n") for c in recorded for s in c["sigs"].values())))


if __name__ == "__main__":
    main_()
