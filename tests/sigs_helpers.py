"""Shared by tests/test_sigs_text.py, tests/test_cli.py and scripts/sigs_text_stage.py: signature rows as a context's pool, name pool and
sequence pool (the state call_bam's tasks leave), the kept rebuild by name over it, and that rebuild downloaded for the host twin."""
import numpy as np

from cutesv_amd import rebuild
from cutesv_amd.columns import BND_CODE, TYPES

NAME_COL = {"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}
STRANDS = ("++", "--")


def case_rows(per, chroms):
    """the reference's candidate tuples {type: [tuple]} -> dict(seg, a, b, aux: lists by row; names: bytes by row; seqs / halves: {row: ..} of
    the INS rows) over the chromosomes `chroms` (sorted: index = name rank)"""
    cidx = {c: i for i, c in enumerate(chroms)}
    n = len(chroms)
    r = dict(seg=[], a=[], b=[], aux=[], names=[], seqs={}, halves={})
    for ti, t in enumerate(TYPES):
        for x in per.get(t, []):
            row = len(r["a"])
            r["seg"].append(ti * n + cidx[x[-1]]); r["names"].append(x[NAME_COL[t]].encode())
            if t in ("DEL", "DUP"):
                r["a"].append(int(x[0])); r["b"].append(int(x[1])); r["aux"].append(0)
            elif t == "INS":
                r["a"].append(int(x[0])); r["b"].append(int(x[1])); r["aux"].append(len(x[3]))
                r["seqs"][row] = x[3]; r["halves"][row] = int(x[0] != int(x[0]))
            elif t == "INV":
                r["a"].append(int(x[1])); r["b"].append(int(x[2])); r["aux"].append(STRANDS.index(x[0]))
            else:
                r["a"].append(int(x[1])); r["b"].append(int(x[3])); r["aux"].append(cidx[x[2]] * 8 + BND_CODE[x[0]])
    return r


def fill_pools(ctx, rows):
    """the rows of case_rows into the context's pools: every row brings its own name (name index = row: the ranks fold the repeats)"""
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    n = len(rows["a"])
    ln = np.asarray([len(x) for x in rows["names"]], np.int32)
    off = np.cumsum(ln, dtype=np.int64) - ln
    assert rebuild.name_pool_append(ctx, b"".join(rows["names"]), off, ln) == 0
    rebuild.pool_append(ctx, rows["seg"], rows["a"], rows["b"], np.arange(n, dtype=np.int32), rows["aux"])
    ins = sorted(rows["seqs"])
    if ins:
        rebuild.seq_pool_put(ctx, ins, [rows["seqs"][k] for k in ins], [rows["halves"].get(k, 0) for k in ins])


def host_rebuild(ctx, n_chrom):
    """the pools' rebuild by name with the ties from the sequences, downloaded: -> (columns dict, first) for sigs_text_host"""
    _, _, major, nodedup = rebuild._segments(["%09d" % k for k in range(n_chrom)], True)
    r = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=False, ties="seqs")
    assert r["n_ins_ties"] == 0
    return r, rebuild.name_ranks(ctx)["first"]


def kept_rebuild(ctx, n_chrom):
    """the same rebuild with its columns kept on the device: what sigs_text / write_sigs read"""
    _, _, major, nodedup = rebuild._segments(["%09d" % k for k in range(n_chrom)], True)
    r = rebuild.rebuild_pool_by_name(ctx, major, nodedup, keep_on_device=True, ties="seqs")
    assert r["n_ins_ties"] == 0
    return r
