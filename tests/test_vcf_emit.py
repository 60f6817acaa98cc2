"""CPU test: the native VCF record emitter (cutesv_amd/csrc/vcf_emit.cpp, no GPU work) against the lines the
reference's generate_output + main_ctrl numbering produce for the same calls (tests/golden/vcf_lines.json.gz)."""

import numpy as np
import pytest

from cutesv_amd import synth, vcf, rows as rows_mod
from cutesv_amd.columns import Params
from oracle import oracle
from helpers import load_json, store_from_json


def _first_diff(a, b):
    la, lb = a.split("\n"), b.split("\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return "line %d:\n got %s\nwant %s" % (i, x[:400], y[:400])
    return "line counts %d vs %d" % (len(la), len(lb))


def _canon(text):
    """DUP / BND read-name lists come from Python sets in the reference (cuteSV_resolveDUP.py:82,96,
    cuteSV_resolveTRA.py:182): their order depends on the interpreter's hash seed, so sort them."""
    out = []
    for line in text.split("\n"):
        if ";RNAMES=" in line and ("SVTYPE=DUP" in line or "SVTYPE=BND" in line):
            head, rest = line.split(";RNAMES=", 1)
            cut = min([i for i in (rest.find(";"), rest.find("\t")) if i >= 0])
            line = head + ";RNAMES=" + ",".join(sorted(rest[:cut].split(","))) + rest[cut:]
        out.append(line)
    return "\n".join(out)


def test_vcf_text_identical_to_reference():
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    golden = load_json("vcf_lines.json.gz")
    assert len(golden) >= 21
    for g in golden:
        case = small[g["case"]]
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        tasks = [(t, c) for t, c, _ in case["rows"]]
        # the order main_ctrl concatenates results in: DEL, INS, INV, DUP, TRA (already the fixture's order)
        hb = st.host_batch(tasks, p)
        res = oracle.cluster_batch(hb, per_sig=False)          # the emitter only sees the SoA; any engine will do
        text, svid = vcf.emit_records(st, hb.segments, res, ref, min_size=p.min_size, max_size=p.max_size,
                                      genotype=p.genotype, **g["flags"])
        assert _canon(text) == _canon(g["text"]), "%s %s: %s" % (g["case"], g["flags"], _first_diff(_canon(text), _canon(g["text"])))
        assert int(svid.sum()) == g["text"].count("\n")


def test_vcf_text_of_genotyped_bnd_records():
    for case in load_json("tra_genotype.json.gz"):
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        ref = {c: synth.reference_sequence(int(st.contig_len[i]), seed=case["vcf"]["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        hb = st.host_batch([(t, c) for t, c, _ in case["rows"]], p)
        res = oracle.cluster_batch(hb, per_sig=False)
        text, svid = vcf.emit_records(st, hb.segments, res, ref, min_size=p.min_size, max_size=p.max_size,
                                      genotype=True, report_readid=True)
        want = case["vcf"]["text"]
        assert _canon(text) == _canon(want), "%s: %s" % (case["name"], _first_diff(_canon(text), _canon(want)))


def test_svid_counters_continue_across_calls():
    case = load_json("small_cases.json.gz")[0]
    st = store_from_json(case["store"])
    p = Params(**case["params"])
    ref = {c: synth.reference_sequence(1_300_000, seed=7 + i) for i, c in enumerate(st.chroms)}
    hb = st.host_batch(st.tasks(), p)
    res = oracle.cluster_batch(hb)
    t1, sv = vcf.emit_records(st, hb.segments, res, ref, min_size=p.min_size, max_size=p.max_size)
    t2, sv = vcf.emit_records(st, hb.segments, res, ref, min_size=p.min_size, max_size=p.max_size, svid=sv)
    n = t1.count("\n")
    assert t2.count("\n") == n and int(sv.sum()) == 2 * n
    assert "cuteSV.DEL.0\t" in t1 and "cuteSV.DEL.0\t" not in t2


def test_fasta_reader(tmp_path):
    from cutesv_amd.fasta import read_fasta
    p = tmp_path / "r.fa"
    p.write_text(">chr1 desc\nACGT\nNNAC\n>chr2\nGG\n\n>chr3\n")
    assert read_fasta(str(p)) == {"chr1": "ACGTNNAC", "chr2": "GG", "chr3": ""}
    assert read_fasta(str(p), only={"chr2"}) == {"chr2": "GG"}


def _write_fasta(path, seqs, width, newline="\n"):
    with open(path, "w", newline="") as f:
        for name, s in seqs.items():
            f.write(">%s some description%s" % (name, newline))
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + newline)


def test_fasta_index_and_mapped_reference(tmp_path):
    """fasta.Reference: the native indexer (csv_fasta_index) gives what `samtools faidx` would (name, length, offset, bases per
    line, bytes per line), an existing .fai is read instead, and fetch() returns the contigs' bases; files that cannot be
    indexed are refused"""
    import pytest
    from cutesv_amd.fasta import Reference, read_fasta
    seqs = {"chr1": synth.reference_sequence(1000, seed=1), "chr2": synth.reference_sequence(61, seed=2), "chrE": "", "chr3": "ACGTN" * 24}
    for width, nl in ((60, "\n"), (7, "\n"), (50, "\r\n")):
        fa = tmp_path / ("w%d%d.fa" % (width, len(nl)))
        _write_fasta(fa, seqs, width, nl)
        ref = Reference(str(fa), write_fai=True)
        assert ref.names == list(seqs)
        assert ref.length.tolist() == [len(s) for s in seqs.values()]
        for i, (n, s) in enumerate(seqs.items()):
            if s:
                assert int(ref.line_bases[i]) == min(width, len(s)) and int(ref.line_width[i]) == min(width, len(s)) + len(nl)
            assert ref.fetch(n) == s and ref.fetch(n, 5, 70) == s[5:70]
        again = Reference(str(fa))                               # through the .fai this time
        assert again.names == ref.names and again.offset.tolist() == ref.offset.tolist() and again.fetch("chr1", 900) == seqs["chr1"][900:]
        assert read_fasta(str(fa)) == seqs
    bad = tmp_path / "bad.fa"
    bad.write_text(">c\nACGT\nAC\nACGT\n")
    with pytest.raises(ValueError):
        Reference(str(bad))


def test_vcf_text_from_a_mapped_fasta_is_the_text_from_strings(tmp_path):
    """REF / ALT bases read in C straight from a memory-mapped FASTA (line_bases / line_width arithmetic) give the records the
    whole-contig strings give - the reference's text (vcf_lines.json.gz) - DEL slices across line breaks and pair types included"""
    from cutesv_amd.fasta import Reference
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    golden = load_json("vcf_lines.json.gz")
    done = 0
    for g in golden:
        if g["flags"].get("ignore_sequence"):
            continue
        case = small[g["case"]]
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        fa = tmp_path / ("ref%d.fa" % done)
        _write_fasta(fa, ref, 60 if done % 2 == 0 else 17)
        mapped = Reference(str(fa))
        tasks = [(t, c) for t, c, _ in case["rows"]]
        hb = st.host_batch(tasks, p)
        res = oracle.cluster_batch(hb, per_sig=False)
        text, _ = vcf.emit_records(st, hb.segments, res, mapped, min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, **g["flags"])
        assert _canon(text) == _canon(g["text"]), "%s %s: %s" % (g["case"], g["flags"], _first_diff(_canon(text), _canon(g["text"])))
        done += 1
        if done >= 8:
            break
    assert done >= 4


# ---------------------------------------------------------------------------------------------- lazy rows (rows.LazyRows)
class _OracleCtx:
    """stands in for engine.Context where only csv_cluster_batch's result matters (the row side is host code)"""

    def cluster_batch(self, hb, reuse=False, **kw):
        return oracle.cluster_batch(hb, per_sig=False)


def _lazy_and_eager(st, p, tasks):
    from cutesv_amd import resolve
    from cutesv_amd.columns import TYPES
    lazy = resolve.cluster_stage(st, p, tasks=tasks, ctx=_OracleCtx(), lazy=True)
    hb = st.host_batch(tasks, p)
    per_seg = rows_mod.rows_by_segment(st, hb.segments, oracle.cluster_batch(hb, per_sig=False))
    eager = {}
    for t in TYPES:
        for k, (tt, ch) in enumerate(tasks):
            if tt == t:
                eager.setdefault(ch, []).extend(per_seg[k])
    return lazy, eager


def test_lazy_rows_are_the_row_lists():
    """cluster_stage(lazy=True) hands out list-like objects backed by the structure of arrays: same rows, same order, and
    everything main_ctrl / generate_output do with a task's rows (extend, sort by int(row[2]), iterate, index: main script
    :1191-1197, GT:242-252) gives what the plain lists give - the str objects just do not exist until somebody looks"""
    from cutesv_amd.rows import LazyRows
    n_checked = 0
    for case in load_json("small_cases.json.gz"):
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        tasks = [(t, c) for t, c, _ in case["rows"]]
        lazy, eager = _lazy_and_eager(st, p, tasks)
        assert set(lazy) == set(eager)
        for ch in eager:
            lz, ea = lazy[ch], eager[ch]
            assert isinstance(lz, LazyRows) and len(lz) == len(ea) and lz.backing() is not None
            assert lz == ea and list(lz) == ea and lz.materialise() == ea
            if ea:
                assert lz[0] == ea[0] and lz[-1] == ea[-1] and lz[len(ea) // 2] == ea[len(ea) // 2] and lz[1:3] == ea[1:3]
                with pytest.raises(IndexError):
                    lz[len(ea)]
            # generate_output's sort: stable, by int(row[2]); from the bp1 column, no strings
            a, b = LazyRows(), list(ea)
            a.extend(lz)
            a.sort(key=lambda x: int(x[2])); b.sort(key=lambda x: int(x[2]))
            assert a.backing() is lz.backing() and a == b
            a.sort(key=lambda x: int(x[2]), reverse=True); b.sort(key=lambda x: int(x[2]), reverse=True)
            assert a == b
            # any other key: the rows are materialised and sorted like a list
            a.sort(key=lambda x: (x[1], len(x))); b.sort(key=lambda x: (x[1], len(x)))
            assert a == b and a.backing() is None
            # mixing with plain rows (tra_bam.genotype_rows returns lists)
            c, d = LazyRows(), []
            c.extend(lz); d.extend(ea)
            extra = [["9", "DEL", "5", "-40", "3", "-1,1", "-2,2", ".", "./.", ".,.,.", ".", ".", "r1,r2"]]
            c.extend(extra); d.extend(extra)
            c.extend(lz); d.extend(ea)
            assert c == d and len(c) == len(d)
            c.sort(key=lambda x: int(x[2])); d.sort(key=lambda x: int(x[2]))
            assert c == d
            n_checked += len(ea)
    assert n_checked > 500


class _RecyclingCtx(_OracleCtx):
    """... and recycles ONE result object the way engine.Context does with reuse=True (overwriting it), with the same lend /
    give_back protocol"""

    def __init__(self):
        self._res_cache, self.made = None, 0

    def cluster_batch(self, hb, reuse=False, **kw):
        fresh = oracle.cluster_batch(hb, per_sig=False)
        if self._res_cache is None:
            self._res_cache, self.made = fresh, self.made + 1
            return fresh
        old = self._res_cache                         # overwrite the recycled arrays in place
        for k, v in fresh.arrays.items():
            if v is not None and old.arrays.get(k) is not None and len(old.arrays[k]) >= len(v):
                old.arrays[k][:len(v)] = v
        old.c.n_calls, old.c.n_support, old.c.n_clusters = fresh.n_calls, fresh.n_support, fresh.n_clusters
        return old



def test_lazy_rows_keep_a_lent_result_instead_of_copying_it():
    """rows.RowsBacking asks the context to lend its recycled result (engine.Context.lend / give_back): the rows then read
    the arrays in place, the context's next call gets other arrays, and a dead backing returns its result"""
    import gc
    from cutesv_amd import resolve, engine
    st = synth.small_mixed(seed=77, genotype=False)
    p = Params.ont()
    tasks = st.tasks()
    ctx = _RecyclingCtx()
    ctx.lend = lambda res: engine.Context.lend(ctx, res)
    ctx.give_back = lambda res: engine.Context.give_back(ctx, res)
    _, eager = _lazy_and_eager(st, p, tasks)
    a = resolve.cluster_stage(st, p, tasks=tasks, ctx=ctx, lazy=True)
    held = next(iter(a.values())).backing().res
    assert ctx._res_cache is None and ctx.made == 1             # lent: no copy was made, the slot is empty
    st2 = synth.small_mixed(seed=78, genotype=False)              # another batch through the same context ...
    b = resolve.cluster_stage(st2, p, tasks=st2.tasks(), ctx=ctx, lazy=True)
    assert ctx.made == 2 and next(iter(b.values())).backing().res is not held
    for ch in eager:                                              # ... leaves the first rows alone
        assert a[ch] == eager[ch]
    del a
    gc.collect()
    assert ctx._res_cache is held                                 # given back
    # a context without the protocol: the rows take a private copy, as before
    c = resolve.cluster_stage(st, p, tasks=tasks, ctx=_OracleCtx(), lazy=True)
    for ch in eager:
        assert c[ch] == eager[ch]


def test_native_emitter_reads_the_lazy_stage_without_rows():
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    for g in load_json("vcf_lines.json.gz")[:9]:
        case = small[g["case"]]
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        tasks = [(t, c) for t, c, _ in case["rows"]]
        from cutesv_amd import resolve
        lazy = resolve.cluster_stage(st, p, tasks=tasks, ctx=_OracleCtx(), lazy=True)
        text, svid = vcf.emit_stage(lazy, ref, min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, **g["flags"])
        assert _canon(text) == _canon(g["text"]), "%s %s" % (g["case"], g["flags"])


def test_reference_generate_output_consumes_lazy_rows():
    """what the reference's generate_output (cuteSV_genotype.py:242-467) does with a chromosome's rows - sorts them in place by
    int(row[2]), iterates them, reads every field of every row - gives, on the LazyRows of cluster_stage(lazy=True), exactly the
    rows the reference handed to it for the cases whose text vcf_lines.json.gz holds (the tasks' rows of small_cases.json.gz,
    concatenated per chromosome in main_ctrl's order); the native emitter writes that text from the same sorted stage"""
    from cutesv_amd import resolve
    from cutesv_amd.columns import TYPES
    from cutesv_amd.rows import LazyRows
    from helpers import READS_FIELD, canonical_row

    def canon(row):
        return canonical_row(row[1] if row[1] in READS_FIELD else "TRA", row)
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    n = n_rows = 0
    for g in load_json("vcf_lines.json.gz"):
        case = small[g["case"]]
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        tasks = [(t, c) for t, c, _ in case["rows"]]
        results = resolve.cluster_stage(st, p, tasks=tasks, ctx=_OracleCtx(), lazy=True)
        want = {}
        for t in TYPES:
            for tt, c, rows in case["rows"]:
                if tt == t:
                    want.setdefault(c, []).extend(rows)
        assert set(results) == set(want), g["case"]
        for c in sorted(results):
            semi = results[c]
            assert isinstance(semi, LazyRows)
            semi.sort(key=lambda x: int(x[2]))
            got = [canon([i[k] for k in range(len(i))]) for i in semi]
            ref_rows = sorted(want[c], key=lambda x: int(x[2]))
            assert got == [canon(r) for r in ref_rows], "%s %s chr%s" % (g["case"], g["flags"], c)
            n_rows += len(got)
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        text, _ = vcf.emit_stage(results, ref, min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, **g["flags"])
        assert _canon(text) == _canon(g["text"]), "%s %s" % (g["case"], g["flags"])
        n += 1
    assert n >= 21 and n_rows > 500


def _count_rows(rows):
    return len(rows), rows[0][2] if len(rows) else None


def test_lazy_rows_pickle_and_the_rest_of_the_list_protocol():
    """main_ctrl hands results[chrom] to Pool.starmap_async(generate_output, ...) (main script :1208-1237), which pickles it: a
    LazyRows travels as the plain list of its rows.  append / insert / + / item assignment / deletion turn it into plain
    rows and behave like a list's (advisor, r05)."""
    import multiprocessing as mp
    import pickle
    from cutesv_amd.rows import LazyRows, BY_POS
    case = next(c for c in load_json("small_cases.json.gz") if c["name"] == "ont_gt")
    st = store_from_json(case["store"])
    p = Params(**case["params"])
    tasks = [(t, c) for t, c, _ in case["rows"]]
    lazy, eager = _lazy_and_eager(st, p, tasks)
    ch = max(eager, key=lambda c: len(eager[c]))
    lz, ea = lazy[ch], eager[ch]
    assert len(ea) > 5
    back = pickle.loads(pickle.dumps(lz))
    assert type(back) is list and back == ea
    with mp.get_context("fork").Pool(2) as pool:                       # the hand-off itself
        got = pool.starmap(_count_rows, [(lz,), (lazy[next(iter(lazy))],)])
    assert got[0] == (len(ea), ea[0][2])
    extra = ["9", "DEL", "5", "-40", "3", "-1,1", "-2,2", ".", "./.", ".,.,.", ".", ".", "r1,r2"]
    a, b = lz.copy(), list(ea)
    assert (a + [extra]) == (b + [extra]) and ([extra] + a) == ([extra] + b) and isinstance(a + [extra], LazyRows)
    a.append(extra); b.append(extra)
    assert a == b and len(a) == len(b) and extra in a and a.index(extra) == b.index(extra) and a.count(extra) == 1
    a.insert(1, extra); b.insert(1, extra)
    a[0] = extra; b[0] = extra
    del a[2]; del b[2]
    assert a == b
    assert a.pop() == b.pop() and a.pop(0) == b.pop(0) and a == b
    a.reverse(); b.reverse()
    assert a == b and bool(a)
    a.remove(extra); b.remove(extra)
    assert a == b
    a.clear()
    assert len(a) == 0 and not a and lz == ea                          # (the copy was the one that changed)
    # the explicit position key: from the bp1 column, no row built; a look-alike key that reads another field as well is not
    # mistaken for it
    c, d = lz.copy(), list(ea)
    c.sort(key=BY_POS); d.sort(key=lambda x: int(x[2]))
    assert c == d and c.backing() is not None
    c.sort_by_pos(reverse=True); d.sort(key=lambda x: int(x[2]), reverse=True)
    assert c == d
    tricky = lambda x: int(x[2]) + (0 if x[4] != "0" else 10 ** 9)      # noqa: E731  (int(row[2]) on every real row)
    c, d = lz.copy(), list(ea)
    c.sort(key=tricky); d.sort(key=tricky)
    assert c == d and c.backing() is None
