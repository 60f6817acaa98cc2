"""Shared by tests/test_ins_seq_pool.py and scripts/ins_seq_stage.py: the cases of rebuild_order.json.gz as rows of a context's
signature pool with their INS sequences put beside them."""
import numpy as np

from cutesv_amd import rebuild
from cutesv_amd.columns import TYPES
from helpers import rebuild_case_inputs


def rebuild_case_pool(ctx, case):
    """a rebuild_order.json.gz case as pool rows (+ the INS sequences beside them) -> (flat list of (type, tuple) by pool row, chroms, ranks, major, nodedup, seqs, halves)"""
    from cutesv_amd.columns import intern_names, BND_CODE
    per, reads = rebuild_case_inputs(case)
    chroms = sorted({x[-1] for t in per for x in per[t]} | {x[2] for x in per["TRA"]} | {r[-1] for r in reads})
    cidx = {c: i for i, c in enumerate(chroms)}
    npos = {"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}
    uniq, _ = intern_names([x[npos[t]] for t in per for x in per[t]] + [r[3] for r in reads])
    rank = {n: i for i, n in enumerate(uniq)}
    strands = sorted({x[0] for x in per["INV"]})
    n = len(chroms)
    flat, seg, a, b, rd, aux = [], [], [], [], [], []
    for ti, t in enumerate(TYPES):
        for x in per.get(t, []):
            flat.append((t, x)); seg.append(ti * n + cidx[x[-1]]); rd.append(rank[x[npos[t]]])
            if t in ("DEL", "DUP"):
                a.append(int(x[0])); b.append(int(x[1])); aux.append(0)
            elif t == "INS":
                a.append(int(x[0])); b.append(int(x[1])); aux.append(len(x[3]))
            elif t == "INV":
                a.append(int(x[1])); b.append(int(x[2])); aux.append(strands.index(x[0]))
            else:
                a.append(int(x[1])); b.append(int(x[3])); aux.append(cidx[x[2]] * 8 + BND_CODE[x[0]])
    major, nodedup = np.zeros(len(TYPES) * n, np.uint8), np.zeros(len(TYPES) * n, np.uint8)
    for ti, t in enumerate(TYPES):
        major[ti * n:(ti + 1) * n] = t in ("INV", "TRA")
        nodedup[ti * n:(ti + 1) * n] = t == "INS"
    rebuild.pool_reset(ctx)
    rebuild.pool_append(ctx, seg, a, b, rd, aux)
    ins_rows = [k for k, (t, _) in enumerate(flat) if t == "INS"]
    seqs = {k: flat[k][1][3] for k in ins_rows}
    halves = {k: int(flat[k][1][0] != int(flat[k][1][0])) for k in ins_rows}
    rebuild.seq_pool_put(ctx, ins_rows, [seqs[k] for k in ins_rows], [halves[k] for k in ins_rows])
    return flat, np.arange(len(uniq), dtype=np.int32), major, nodedup, seqs, halves
