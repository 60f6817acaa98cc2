"""The split-read analysis (cutesv_amd/csrc/split.hip.h) at its thresholds, and the slice bounds of its INS candidates where they
leave [0, read length]: crafted reads against the lists the reference's organize_split_signal / analysis_split_read recorded for
them (tests/golden/split_edges.json.gz, made by make_golden_split.split_edges).

A family of the fixture is one base read with one quantity moved across a rule's threshold; coordinates are a few hundred, so
comparisons land on equality and a slice c:d of an INS candidate can start below 0, end behind the read or be empty.  Such a
slice has Python's meaning wherever it becomes a length (the pool row's aux) or bytes (the sequence pool).

CPU: the oracle and the host twins against the recorded lists, and what the fixture itself covers.  GPU: csv_split_signatures on
every case, reads on either side of a thread-block seam, a random small-coordinate batch against the oracle, the pool rows, the
sequence pool with stored-forward and stored-reversed reads, and the same reads as BAM records through task_to_pool.
Every comparison is an exact integer or byte comparison."""
import collections

import numpy as np
import pytest

from cutesv_amd import bam, extract, rebuild, synth
from cutesv_amd.columns import TYPES, BND_CODE, SigStore
from helpers import load_json, split_case_inputs, assert_split_case
import bam_writer

KINDS = ("DEL", "INS", "DUP", "INV", "TRA")
SPLIT_KEYS = ("kind", "read", "chr", "aux", "a", "b", "c", "d")
NAME_POS = {"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}
CODES = "=ACMGRSVTWYHKDBN"
_PACK = bytes.maketrans(CODES.encode(), bytes(range(16)))
# every family the fixture must hold, by the rule of the analysis it aims at
FAMILIES = {
    "organize": ("org_mapq", "org_no_primary", "org_parts", "org_n01", "org_equal_rs2", "org_equal_rs3"),
    "two-segment INV": ("inv2_branch1_sv", "inv2_branch2_sv", "inv2_branch3_sv", "inv2_branch4_sv", "inv2_half_even", "inv2_half_odd", "inv2_half_minus_odd"),
    "BND": ("bnd_gap", "bnd_shapes"),
    "two segments, one strand": ("two_overlap_sv", "two_overlap_sv_minus", "two_ins_or_dup", "two_ins_or_dup_minus"),
    "INS / DEL pair": ("indel_ins_delta_sv", "indel_ins_delta_sv_minus", "indel_del_delta_sv", "indel_del_delta_sv_minus", "indel_ins_overlap_fifth",
                       "indel_del_overlap_fifth", "indel_ins_overlap_fifth_31", "indel_del_overlap_fifth_31", "indel_ins_gap_100", "indel_del_gap_100",
                       "indel_ins_gap_fifth", "indel_del_gap_fifth", "indel_ins_max", "indel_del_max", "indel_trunc_negative", "indel_trunc_negative_minus",
                       "indel_trunc_positive", "indel_trunc_positive_minus", "indel_half_position"),
    "three segments": ("tri_pmp_first_even", "tri_pmp_first_odd", "tri_pmp_second_even", "tri_pmp_second_odd", "tri_pmp_gate_first", "tri_pmp_gate_second",
                       "tri_mpm_first_even", "tri_mpm_first_odd", "tri_mpm_second_even", "tri_mpm_second_odd", "tri_mpm_gate_first", "tri_mpm_gate_second"),
    "last window": ("lastwin_choice", "lastwin_fourth"),
    "one strand": ("one_dup_sv", "one_dup_sv_minus", "one_dup_gate", "one_dup_first_window", "one_gate_third", "one_gate_third_minus", "one_last_extra"),
    "routes": ("route_third_none_plus", "route_third_none_minus", "route_pair_then_other_plus", "route_pair_then_other_minus"),
    "insertion inside a translocation": ("instra_ref_distance", "instra_ref_distance_minus", "instra_ref_distance_negative", "instra_ref_distance_negative_minus",
                                         "instra_ref_distance_fifth", "instra_length_sv", "instra_length_max", "instra_min_side", "instra_ends_differ"),
    "slices": ("slice_negative_start_plus", "slice_negative_start_minus", "slice_negative_start_reversed_record", "slice_negative_start_forward_record",
               "slice_negative_start_two_segment_rule", "slice_end_past_read_plus", "slice_end_past_read_minus", "slice_end_past_read_reversed_record",
               "slice_end_past_read_forward_record", "slice_start_past_read_plus", "slice_start_past_read_minus", "slice_negative_end_plus",
               "slice_negative_end_minus", "slice_empty_plus", "slice_empty_minus"),
}
# the parameter sets of test_hip_parity's random-batch test
PARAM_SETS = (dict(sv_size=30, min_mapq=20, max_split_parts=7, max_size=100000), dict(sv_size=1, min_mapq=0, max_split_parts=-1, max_size=-1),
              dict(sv_size=200, min_mapq=30, max_split_parts=3, max_size=5000), dict(sv_size=0, min_mapq=61, max_split_parts=12, max_size=100))


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """the fixture's cases with their inputs and the oracle's candidate arrays, made once: (case, enc, names, queries, chroms, kw, sig)"""
    out = []
    for case in load_json("split_edges.json.gz"):
        enc, names, queries, chroms, kw = split_case_inputs(case)
        out.append((case, enc, names, queries, chroms, kw, _oracle().split_signatures(enc, **kw)))
    return out


def revcomp(s):
    return s.translate(extract._COMP)[::-1]


def pack4(seqs):
    """sequences -> (uint8 image, off int64[n], l_seq int32[n]) in the BAM 4-bit encoding, high nibble first"""
    parts, off, at = [], [], 0
    for s in seqs:
        codes = s.encode().translate(_PACK) + b"\0"
        p = bytes(hi << 4 | lo for hi, lo in zip(codes[0:len(s):2], codes[1:len(s) + 1:2]))
        parts.append(p); off.append(at); at += len(p)
    return np.frombuffer(b"".join(parts) + b"\0", np.uint8), np.asarray(off, np.int64), np.asarray([len(s) for s in seqs], np.int32)


def reference_ins(case):
    """[(inserted sequence, x.5 flag)] of the reference's INS tuples"""
    return [(x[3], int(x[0] != int(x[0]))) for x in case["INS"]]


def reference_rows(case, sig, names, chroms):
    """the pool rows of the reference's tuples in candidate order - the encoding of columns.from_tuple_lists: (kind, chr rank, a, b, read, aux)"""
    rank = {c: i for i, c in enumerate(chroms)}
    index = {n: i for i, n in enumerate(names)}
    at = {t: 0 for t in KINDS}
    rows = []
    for kind in sig["kind"].tolist():
        t = KINDS[kind]
        x = case[t][at[t]]; at[t] += 1
        read = index[x[NAME_POS[t]]]
        if t in ("DEL", "DUP"):
            rows.append((kind, rank[x[-1]], int(x[0]), int(x[1]), read, 0))
        elif t == "INS":
            rows.append((kind, rank[x[-1]], int(x[0]), int(x[1]), read, len(x[3])))
        elif t == "INV":
            rows.append((kind, rank[x[-1]], int(x[1]), int(x[2]), read, {"++": 0, "--": 1}[x[0]]))
        else:
            rows.append((kind, rank[x[-1]], int(x[1]), int(x[3]), read, rank[x[2]] * 8 + BND_CODE[x[0]]))
    assert all(at[t] == len(case[t]) for t in KINDS)
    return rows


def store_rows(per_type, chroms):
    """columns.from_tuple_lists on candidate tuples -> the set of its rows as (type, chr, a, b, read name, aux), the INV strand as 0 / 1"""
    st = SigStore.from_tuple_lists({t: [tuple(x) for x in per_type[t]] for t in KINDS}, chroms=chroms)
    rows = set()
    for (t, ch), (b, e) in st.seg_index.items():
        for i in range(b, e):
            aux = int(st.aux[i])
            rows.add((t, ch, int(st.a[i]), int(st.b[i]), st.names[st.read_id[i]], ("++", "--").index(st.strands[aux]) if t == "INV" else aux))
    return rows


def pool_columns(ctx, n_seg):
    """the pool's rows in pool order, through a rebuild that keeps every row"""
    n = rebuild.pool_rows(ctx)
    ident = np.arange(1 << 16, dtype=np.int32)
    r = rebuild.rebuild_pool(ctx, ident, np.zeros(n_seg, np.uint8), np.ones(n_seg, np.uint8), keep_on_device=False)
    assert r["n_out"] == n
    back = np.argsort(r["src_row"], kind="stable")
    return {k: r[k][back] for k in ("seg_id", "a", "b", "read_id", "aux")}


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_equals_the_reference_on_every_case():
    cases = load_json("split_edges.json.gz")
    assert [c["name"] for c in cases] == ["edges", "edges_tight", "edges_no_limits", "edges_sv0"] + ["small_fuzz_%d" % k for k in range(6)]
    kinds = set()
    for case in cases:
        sig = assert_split_case(case, _oracle().split_signatures)
        kinds |= set(np.unique(sig["kind"]).tolist())
    assert kinds == {0, 1, 2, 3, 4}


def test_fixture_covers_every_family_and_the_slices_that_leave_the_read(cases):
    """from the fixture's own recorded lists and its family / step fields"""
    by_family = collections.defaultdict(list)
    neg_start = past_end = empty = neg_start_fuzz = 0
    for case, enc, names, queries, chroms, kw, sig in cases:
        per_read = {n: {t: [] for t in KINDS} for n in names}
        for t in KINDS:
            for x in case[t]:
                per_read[x[NAME_POS[t]]][t].append(x)
        for r in case["reads"]:
            by_family[r["family"]].append((r["step"], per_read[r["name"]]))
        ins = sig["kind"] == 1
        L = np.asarray([r["qlen"] for r in case["reads"]], np.int64)[sig["read"][ins]]
        neg_start += int((sig["c"][ins] < 0).sum())
        neg_start_fuzz += int((sig["c"][ins] < 0).sum()) if case["name"].startswith("small_fuzz") else 0
        past_end += int((sig["d"][ins] > L).sum())
        empty += sum(1 for x in case["INS"] if x[3] == "")
    want = {f for group in FAMILIES.values() for f in group}
    assert want <= set(by_family), sorted(want - set(by_family))
    assert set(by_family) == want | {"small_fuzz"}
    for fam in sorted(want):
        outs = [o for _, o in by_family[fam]]
        assert len(outs) >= 2 and any(x != y for x, y in zip(outs, outs[1:])), fam
    assert neg_start_fuzz >= 5 and neg_start >= 5 and past_end >= 1 and empty >= 1, (neg_start_fuzz, neg_start, past_end, empty)
    ins = [x for case, *_ in cases for x in case["INS"]]
    assert any(type(x[0]) is float for x in ins) and any(type(x[0]) is int for x in ins)
    assert sum(len(c[0]["reads"]) for c in cases if c[0]["name"].startswith("small_fuzz")) == 3000


def test_host_pool_rows_carry_the_length_of_the_reference_sequence(cases):
    """extract.pool_rows_of_split: the aux of a kind-1 row is len(sequence) of the reference's tuple, and every row is what
    columns.from_tuple_lists makes of the reference's tuples"""
    n_neg = 0
    for case, enc, names, queries, chroms, kw, sig in cases:
        rows = extract.pool_rows_of_split(sig, [100 * k for k in range(5)], 7000, [len(q) for q in queries])
        ins = sig["kind"] == 1
        assert rows["aux"][ins].tolist() == [len(x[3]) for x in case["INS"]], case["name"]
        want = reference_rows(case, sig, names, chroms)
        got = list(zip(((rows["seg"] // 100).tolist()), (rows["seg"] % 100).tolist(), rows["a"].tolist(), rows["b"].tolist(), (rows["read"] - 7000).tolist(),
                       rows["aux"].tolist()))
        assert got == want, case["name"]
        assert {(KINDS[k], chroms[c], a, b, names[r], x) for k, c, a, b, r, x in got} == store_rows(case, chroms), case["name"]
        n_neg += int((sig["c"][ins] < 0).sum())
    assert n_neg >= 40


def test_host_sequences_equal_the_reference_strings(cases):
    """extract.pool_ins_sequences_host with the reads stored forward, stored reversed and half and half"""
    for case, enc, names, queries, chroms, kw, sig in cases:
        want = reference_ins(case)
        n = len(queries)
        for rev in ([0] * n, [1] * n, [k & 1 for k in range(n)]):
            stored = [revcomp(q) if r else q for q, r in zip(queries, rev)]
            got = extract.pool_ins_sequences_host(stored, rev, None, sig)
            assert [(b.decode(), h) for b, h in got] == want, case["name"]


# ------------------------------------------------------------------------------------------------ GPU: csv_split_signatures
@pytest.mark.gpu
def test_gpu_direct_call_equals_the_reference_and_the_oracle(ctx, cases):
    for case, enc, names, queries, chroms, kw, want in cases:
        got = assert_split_case(case, lambda e, **k: extract.split_signatures(ctx, e, **k))
        for k in SPLIT_KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (case["name"], k)


def spread(enc, n_batch, shift):
    """the reads of `enc`, rotated by `shift`, as the LAST reads of a batch of n_batch: the reads in front of them have no entry"""
    n = len(enc["read_len"])
    order = (np.arange(n) + shift) % n
    cnt = np.diff(enc["ent_off"])[order]
    pick = np.concatenate([np.arange(enc["ent_off"][r], enc["ent_off"][r + 1]) for r in order.tolist()]).astype(np.int64)
    out = {k: enc[k][pick] for k in ("c0", "c1", "f0", "f1", "chr", "mapq", "strand", "primary")}
    pad = n_batch - n
    out["ent_off"] = np.concatenate([np.zeros(pad, np.int64), np.concatenate([[0], np.cumsum(cnt)])]).astype(np.int64)
    out["read_len"] = np.concatenate([np.full(pad, 100, np.int64), enc["read_len"][order]])
    return out, pad, order


@pytest.mark.gpu
@pytest.mark.parametrize("n_batch", (255, 256, 257))
def test_gpu_reads_on_both_sides_of_a_thread_block_seam(ctx, cases, n_batch):
    """crafted reads in the last thread of a 256-thread block and in the first thread of the next"""
    case, enc, names, queries, chroms, kw, want = cases[0]
    keep = min(len(names), 250)
    sub = dict({k: enc[k][:enc["ent_off"][keep]] for k in ("c0", "c1", "f0", "f1", "chr", "mapq", "strand", "primary")},
               ent_off=enc["ent_off"][:keep + 1], read_len=enc["read_len"][:keep])
    ref = _oracle().split_signatures(sub, **kw)
    per_read = [np.flatnonzero(ref["read"] == r) for r in range(keep)]
    for shift in (0, 97):
        batch, pad, order = spread(sub, n_batch, shift)
        assert len(batch["read_len"]) == n_batch and batch["ent_off"][-1] == sub["ent_off"][-1]
        got = extract.split_signatures(ctx, batch, **kw)
        rows = np.concatenate([per_read[r] for r in order.tolist()])          # the candidates of the sub-case in the batch's read order
        back = np.full(keep, -1); back[order] = pad + np.arange(keep)
        for k in SPLIT_KEYS:
            w = back[ref["read"][rows]].astype(np.int32) if k == "read" else ref[k][rows]
            assert np.array_equal(got[k], w), (n_batch, shift, k)
        assert len(got["kind"]) > 100 and got["read"].min() >= pad


def random_small_batch(rng, n_reads, n_chrom=3):
    """flat csv_split_in arrays of random reads with L < 400, reference coordinates below 1000 and 0 .. 6 entries"""
    n_ent = rng.integers(0, 7, n_reads)
    ent_off = np.zeros(n_reads + 1, np.int64); np.cumsum(n_ent, out=ent_off[1:])
    ne = int(ent_off[-1])
    read = np.repeat(np.arange(n_reads), n_ent)
    first = np.zeros(ne, bool); first[ent_off[:-1][n_ent > 0]] = True
    L = rng.integers(150, 400, n_reads).astype(np.int64)
    primary = (first & (rng.random(ne) < 0.85)).astype(np.uint8)
    base_st = np.repeat((rng.random(n_reads) < 0.5).astype(np.uint8), n_ent)
    strand = np.where(rng.random(ne) < 0.75, base_st, 1 - base_st).astype(np.uint8)
    base_ch = np.repeat(rng.integers(0, n_chrom, n_reads), n_ent)
    chrom = np.where(rng.random(ne) < 0.85, base_ch, rng.integers(0, n_chrom, ne)).astype(np.int32)
    Lr = L[read]
    lo = (rng.random(ne) * (Lr - 1)).astype(np.int64); hi = np.minimum(Lr, lo + 1 + (rng.random(ne) * Lr).astype(np.int64))
    base_ref = np.repeat(rng.integers(100, 600, n_reads), n_ent)
    ref = np.maximum(0, base_ref + rng.integers(-120, 160, ne)).astype(np.int64)
    span = rng.integers(1, 200, ne).astype(np.int64)
    c0 = np.where(primary == 1, lo, np.where(strand == 0, lo, Lr - hi)); c1 = np.where(primary == 1, hi, np.where(strand == 0, Lr - hi, lo))
    f1 = np.where(primary == 1, ref + span, span)
    assert int((ref + span).max()) < 1000
    mapq = rng.choice(np.array([0, 3, 20, 30, 60], np.int32), ne)
    return dict(ent_off=ent_off, read_len=L, c0=c0.astype(np.int64), c1=c1.astype(np.int64), f0=ref, f1=f1.astype(np.int64), chr=chrom, mapq=mapq,
                strand=strand, primary=primary)


@pytest.fixture(scope="module")
def small_batch():
    """(the random batch, the oracle's result per parameter set)"""
    enc = random_small_batch(np.random.default_rng(417), 20000)
    return enc, [_oracle().split_signatures(enc, **kw) for kw in PARAM_SETS]


def test_random_small_batch_reaches_the_slices_that_start_below_zero(small_batch):
    _, wants = small_batch
    seen, neg = set(), 0
    for want in wants:
        seen |= set(np.unique(want["kind"]).tolist())
        neg += int(((want["kind"] == 1) & (want["c"] < 0)).sum())
    assert seen == {0, 1, 2, 3, 4} and neg >= 20, (seen, neg)


@pytest.mark.gpu
def test_gpu_random_small_batch_equals_the_oracle(ctx, small_batch):
    enc, wants = small_batch
    seen, neg = set(), 0
    for kw, want in zip(PARAM_SETS, wants):
        got = extract.split_signatures(ctx, enc, **kw)
        for k in SPLIT_KEYS:
            assert np.array_equal(got[k], want[k]), (kw, k, len(got[k]), len(want[k]))
        seen |= set(np.unique(got["kind"]).tolist())
        neg += int(((got["kind"] == 1) & (got["c"] < 0)).sum())
        # ... and the pool rows of such a batch carry Python's slice lengths
        rebuild.pool_reset(ctx)
        n = extract.split_signatures(ctx, enc, pool=dict(seg_base=[0, 3, 6, 9, 12], read_base=0, query_len=enc["read_len"]), host_outputs=False, **kw)["n"]
        rows = extract.pool_rows_of_split(want, [0, 3, 6, 9, 12], 0, enc["read_len"])
        assert n == len(want["kind"])
        if n:
            cols = pool_columns(ctx, 15)
            for a, b in (("seg_id", "seg"), ("a", "a"), ("b", "b"), ("read_id", "read"), ("aux", "aux")):
                assert np.array_equal(cols[a], rows[b]), (kw, a)
    rebuild.pool_reset(ctx)
    assert seen == {0, 1, 2, 3, 4} and neg >= 20, (seen, neg)


# ------------------------------------------------------------------------------------------------ GPU: pool rows and sequences
@pytest.mark.gpu
def test_gpu_pool_rows_equal_the_reference_tuples(ctx, cases):
    seg_base = [0, 4, 8, 12, 16]
    n_neg = 0
    for case, enc, names, queries, chroms, kw, sig in cases:
        rebuild.pool_reset(ctx)
        res = extract.split_signatures(ctx, enc, pool=dict(seg_base=seg_base, read_base=0, query_len=[len(q) for q in queries]), host_outputs=False, **kw)
        want = reference_rows(case, sig, names, chroms)
        assert res["n"] == rebuild.pool_rows(ctx) == len(want)
        cols = pool_columns(ctx, 20)
        got = list(zip((cols["seg_id"] // 4).tolist(), (cols["seg_id"] % 4).tolist(), cols["a"].tolist(), cols["b"].tolist(), cols["read_id"].tolist(), cols["aux"].tolist()))
        assert got == want, (case["name"], next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w))
        assert {(KINDS[k], chroms[c], a, b, names[r], x) for k, c, a, b, r, x in got} == store_rows(case, chroms), case["name"]
        ins = cols["seg_id"] // 4 == 1
        assert cols["aux"][ins].tolist() == [len(x[3]) for x in case["INS"]], case["name"]
        n_neg += int(((sig["kind"] == 1) & (sig["c"] < 0)).sum())
    rebuild.pool_reset(ctx)
    assert n_neg >= 40


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", ("none", "all", "odd", "even"))
def test_gpu_sequence_pool_holds_the_reference_strings(ctx, cases, reverse):
    """the bases and x.5 flags of the INS rows, cut on the device out of reads stored forward or reversed: both values of `rev` in the
    gather cut slices that start below 0 and slices that end behind the read"""
    cut = collections.Counter()
    for case, enc, names, queries, chroms, kw, sig in cases:
        n = len(queries)
        rev = np.asarray([dict(none=0, all=1, odd=k & 1, even=1 - (k & 1))[reverse] for k in range(n)], np.uint8)
        stored = [revcomp(q) if r else q for q, r in zip(queries, rev.tolist())]
        img, s_off, l_seq = pack4(stored)
        rebuild.pool_reset(ctx)
        extract.upload_read_sequences(ctx, img, s_off, l_seq)
        ssig = extract.split_signatures(ctx, enc, pool=dict(seg_base=[0, 4, 8, 12, 16], read_base=0, query_len=l_seq, seqs=True, query_reverse=rev), **kw)   # must not refuse
        for k in SPLIT_KEYS:
            assert np.array_equal(ssig[k], sig[k]), (case["name"], k)
        rows = np.flatnonzero(ssig["kind"] == 1)
        want = reference_ins(case)
        assert rebuild.pool_rows(ctx) == len(ssig["kind"]) and len(rows) == len(want)
        got = rebuild.seq_pool_get(ctx, rows, raw=True)
        assert [g.decode() for g in got] == [s for s, _ in want], case["name"]
        assert rebuild.seq_pool_half(ctx, rows).tolist() == [h for _, h in want], case["name"]
        assert rebuild.seq_pool_rows(ctx) == (len(rows), sum(len(s) for s, _ in want))
        gather_rev = rev[ssig["read"][rows]] != (ssig["aux"][rows] & 1)
        L = np.asarray(l_seq, np.int64)[ssig["read"][rows]]
        for r in (False, True):
            cut[("c<0", r)] += int(((ssig["c"][rows] < 0) & (gather_rev == r)).sum())
            cut[("d>L", r)] += int(((ssig["d"][rows] > L) & (gather_rev == r)).sum())
    rebuild.pool_reset(ctx)
    need = (False,) if reverse == "none" else (True, False) if reverse in ("odd", "even") else ()
    assert all(cut[(w, r)] >= 3 for w in ("c<0", "d>L") for r in need), cut
    assert cut[("c<0", False)] + cut[("c<0", True)] >= 40


# ------------------------------------------------------------------------------------------------ GPU: the BAM route
REFS = [("1", 10 ** 6), ("10", 10 ** 6), ("2", 10 ** 6), ("X", 10 ** 6)]


def bam_records(case):
    """the reads of the `slice_*` and `instra_*` families whose own alignment can be a record (it lies inside the read), as records on
    contig "1": the primary segment becomes flag, clips and a CIGAR with one gap that gives both of its spans; the SA text is the read's"""
    recs = []
    for d, q in zip(case["reads"], split_case_inputs(case)[2]):
        if not d["family"].startswith(("slice_", "instra_")) or not d["primary"]:
            continue
        c0, c1, f0, f1, chrom, strand = d["primary"]
        if not (0 <= c0 and c0 + 2 <= c1 <= d["qlen"]) or chrom != "1":
            continue
        left, right = (c0, d["qlen"] - c1) if strand == "+" else (d["qlen"] - c1, c0)
        q_span, r_span = c1 - c0, f1 - f0
        m = min(q_span, r_span)
        gap = [(2, r_span - q_span)] if r_span > q_span else [(1, q_span - r_span)] if q_span > r_span else []
        cig = ([(4, left)] if left else []) + [(0, m // 2)] + gap + [(0, m - m // 2)] + ([(4, right)] if right else [])
        assert sum(n for o, n in cig if o in (0, 1, 4)) == d["qlen"] and sum(n for o, n in cig if o in (0, 2)) == r_span
        recs.append(dict(name=d["name"], flag=0 if strand == "+" else 16, mapq=60, start=f0, cigar=cig, seq=q if strand == "+" else revcomp(q),
                         tags=[("SA", d["sa"])], refid=0))
    recs.sort(key=lambda r: r["start"])
    return recs


@pytest.mark.gpu
def test_gpu_task_to_pool_on_the_slice_families_as_bam_records(ctx, cases, tmp_path):
    chroms = [n for n, _ in REFS]
    rank = {c: i for i, c in enumerate(chroms)}
    n_chrom = len(chroms)
    seg_of = lambda t, ci: TYPES.index(t) * n_chrom + ci                        # noqa: E731
    seg_base = [seg_of(t, 0) for t in KINDS]
    seen = collections.Counter()
    for case, enc, names, queries, _, kw, sig in cases[:4]:
        recs = bam_records(case)
        if case["name"] == "edges":
            assert len(recs) > 60 and {r["flag"] for r in recs} == {0, 16}
        assert recs, case["name"]
        p = case["params"]
        path = str(tmp_path / (case["name"] + ".bam"))
        bam_writer.write_bam(path, REFS, recs)
        pipe = (p["sv"], p["min_mapq"], p["parts"], 0, 10, 0, 100, p["max_size"])
        with bam.BamFile(path) as bf:
            rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
            res = extract.task_to_pool(ctx, bf, "1", 0, 1 << 40, rank, *pipe, seg_of("INS", 0), seg_of("DEL", 0), seg_base, None, seq_pool=True, name_pool=True)   # must return
            cand, _ = extract.single_pipe_bam((_oracle().cigar_signatures, _oracle().split_signatures), bf, "1", 0, 1 << 40, rank, *pipe)
            ch = bf.records("1", 0, 1 << 40)
        assert res["n_flagged"] == 0 and res["n_records"] == len(recs) == res["n_calls"]
        # the file says what the fixture says: the reference's tuples of these reads are among the candidates of the task
        mine = {r["name"] for r in recs}
        for t in KINDS:
            have = collections.Counter(tuple(x) for x in cand[t])
            need = collections.Counter(tuple(x) for x in case[t] if x[NAME_POS[t]] in mine)
            assert not need - have, (case["name"], t, list((need - have).items())[:3])
            seen[t] += sum(need.values())
        cols = pool_columns(ctx, len(TYPES) * n_chrom)
        assert rebuild.pool_rows(ctx) == sum(len(v) for v in cand.values())
        rec_names = [ch.name(i) for i in range(ch.n)]
        assert rebuild.name_pool_get(ctx, np.arange(ch.n) + res["name_base"]) == rec_names
        got = {(TYPES[s // n_chrom], chroms[s % n_chrom], a, b, rec_names[r - res["name_base"]], x)
               for s, a, b, r, x in zip(cols["seg_id"].tolist(), cols["a"].tolist(), cols["b"].tolist(), cols["read_id"].tolist(), cols["aux"].tolist())}
        assert got == store_rows(cand, chroms), case["name"]
        rows = np.flatnonzero((cols["seg_id"] >= seg_base[1]) & (cols["seg_id"] < seg_base[1] + n_chrom))
        assert res["n_seq_rows"] == len(rows) == len(cand["INS"])
        seqs, half = rebuild.seq_pool_get(ctx, rows), rebuild.seq_pool_half(ctx, rows)
        assert cols["aux"][rows].tolist() == [len(s) for s in seqs]
        have = sorted((rec_names[cols["read_id"][r] - res["name_base"]], int(cols["a"][r]), int(cols["b"][r]), s, int(h)) for r, s, h in zip(rows.tolist(), seqs, half.tolist()))
        assert have == sorted((x[2], int(x[0]), int(x[1]), x[3], int(x[0] != int(x[0]))) for x in cand["INS"]), case["name"]
        seen["empty"] += sum(1 for x in case["INS"] if x[2] in mine and x[3] == "")
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    assert seen["INS"] >= 40 and seen["DUP"] >= 2 and seen["TRA"] >= 40 and seen["empty"] >= 4, seen
