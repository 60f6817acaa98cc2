"""SA tags parsed on the GPU (cutesv_amd/csrc/sa.hip.h, csv_bam_split_inputs): the entry columns the
device makes of a decoded BAM chunk against `extract.encode_split_reads` on the same reads built the old way
(`_primary_info` + `Chunk.sa_values`), the split-read analysis on them in place (CSV_SP_FROM_BAM), `single_pipe_bam(sa="device")`
against the reference's recorded single_pipe output, and `task_to_pool` against the pool rows of the existing path.

The five golden cases (parse_reads.json.gz, single_pipe.json.gz) hold 983 SA tags with 3 217 entries; every one fits the
device's strict grammar, so on them the number of flagged calls must be exactly 0 - each golden test asserts that: the host
fallback cannot hide a broken parser.  The grammar's edges are in a hand-written BAM (edge_records)."""
import ctypes as C

import numpy as np
import pytest

from cutesv_amd import bam, extract, synth, _abi, _lib
from helpers import load_json
import bam_writer

REF_LEN = {"1": 248956422, "10": 133797422, "2": 242193529, "7": 159345973, "X": 156040895}
ENC_KEYS = ("c0", "c1", "f0", "f1", "chr", "mapq", "strand", "primary", "ent_off", "read_len")
SPLIT_KEYS = ("kind", "read", "chr", "aux", "a", "b", "c", "d")


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def golden_records(case, chrom):
    refs = [(c, REF_LEN[c]) for c in case["chroms"]]
    refid = case["chroms"].index(chrom)
    recs = [dict(d, seq=synth.pseudo_sequence(d["seq_len"], d["seq_key"]), refid=refid, tags=[tuple(t) for t in d["tags"]]) for d in case["reads"]]
    return refs, recs


def all_cases():
    return ([(c, c["chrom"]) for c in load_json("parse_reads.json.gz")] + [(c, c["task"][0]) for c in load_json("single_pipe.json.gz")])


def skw(p):
    return dict(sv_size=p["sv"], min_mapq=p["min_mapq"], max_split_parts=p["parts"], max_size=p["max_size"])


def pipe_args(p):
    return (p["sv"], p["min_mapq"], p["parts"], p["min_read_len"], p["min_siglength"], p["md"], p["mi"], p["max_size"])


def selection(cols, min_read_len):
    """the records whose SA tags parse_read looks at: primary, long enough, with a tag"""
    return (cols["query_len"] >= min_read_len) & (cols["cls"] == 1) & (cols["sa_off"][1:] > cols["sa_off"][:-1])


def old_way(chunk, cols, sel, chrom, min_mapq):
    """the split-read inputs as single_pipe_bam builds them on the host: ([(primary_info, SA value, query_length)] per call, record per call)"""
    reads, call_rec = [], []
    for i in np.flatnonzero(sel).tolist():
        primary = extract._primary_info(int(cols["flag"][i]), cols["mapq"][i] >= min_mapq, int(cols["clip_left"][i]), int(cols["clip_right"][i]),
                                        int(cols["query_len"][i]), int(cols["ref_start"][i]), int(cols["ref_end"][i]), chrom)
        for value in chunk.sa_values(cols, i):
            reads.append((primary, value, int(cols["query_len"][i]))); call_rec.append(i)
    return reads, call_rec


def one_chunk(path, chrom):
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks(chrom))
    return ch


# ------------------------------------------------------------------------------------------------ the strict grammar, on the host
def strict_parse(value, rank):
    """What the device parser does with an SA value, character by character and without int() or a regular expression:
    -> the entries [(c0, c1, f0, f1, chr, mapq, strand)] (None when the call is flagged)"""
    out = []
    for entry in value.split(";")[:-1]:
        f = entry.split(",")
        if len(f) < 5 or f[0] not in rank or len(f[2]) != 1:
            return None
        nums = []
        for text, width in ((f[1], 18), (f[4], 9)):
            if not 0 < len(text) <= width or any(ch not in "0123456789" for ch in text):
                return None
            v = 0
            for ch in text:
                v = v * 10 + "0123456789".index(ch)
            nums.append(v)
        ops, v, nd = [], 0, 0
        if f[3] != "*":
            if not f[3]:
                return None
            for ch in f[3]:
                if ch in "0123456789":
                    v, nd = v * 10 + "0123456789".index(ch), nd + 1
                    if nd > 18:
                        return None
                elif ch in "MIDNSHP=XB" and nd:
                    ops.append((v, ch)); v, nd = 0, 0
                else:
                    return None
            if nd:
                return None
        span = sum(n for n, o in ops if o in "MD=X")
        if span > 1 << 62:
            return None
        out.append((ops[0][0] if ops and ops[0][1] == "S" else 0, ops[-1][0] if ops and ops[-1][1] == "S" else 0, nums[0] - 1, span,
                    rank[f[0]], nums[1], 0 if f[2] == "+" else 1))
    return out


def test_abi_has_the_split_input_entries():
    L = _lib.lib()
    assert _abi.ABI_VERSION == 9 and L.csv_abi_version() == 9
    assert hasattr(L, "csv_bam_split_inputs") and hasattr(L, "csv_sa_struct_size")
    assert [L.csv_sa_struct_size(i) for i in range(3)] == [C.sizeof(extract.SaIn), C.sizeof(extract.SaOut), -1]
    assert _abi.SP_FROM_BAM == 4 and _abi.CG_TO_POOL == 1
    assert L.csv_bam_struct_size(3) == -1


def test_device_sa_needs_a_context(tmp_path):
    case = load_json("single_pipe.json.gz")[0]
    refs, recs = golden_records(case, "7")
    path = str(tmp_path / "a.bam")
    bam_writer.write_bam(path, refs, recs[:20])
    o = _oracle()
    rank = {c: i for i, c in enumerate(case["chroms"])}
    with bam.BamFile(path) as bf:
        with pytest.raises(ValueError):
            extract.single_pipe_bam((o.cigar_signatures, o.split_signatures), bf, "7", 0, 1 << 40, rank, *pipe_args(case["params"]), sa="device")
        with pytest.raises(ValueError):
            extract.single_pipe_bam((o.cigar_signatures, o.split_signatures), bf, "7", 0, 1 << 40, rank, *pipe_args(case["params"]), sa="gpu")


def test_strict_grammar_agrees_with_encode_split_reads_on_the_goldens():
    n_tags = n_entries = 0
    for case, chrom in all_cases():
        rank = {c: i for i, c in enumerate(case["chroms"])}
        for d in case["reads"]:
            for t in d["tags"]:
                if t[0] != "SA":
                    continue
                value = t[-1]
                assert value.endswith(";") and extract.sa_status(value, rank) == 0
                want = extract.encode_split_reads([([], value, 1000)], rank)
                got = strict_parse(value, rank)
                assert got is not None and len(got) == int(want["ent_off"][-1])
                for k, col in enumerate(("c0", "c1", "f0", "f1", "chr", "mapq", "strand")):
                    assert [e[k] for e in got] == want[col].tolist(), (value, col)
                n_tags += 1; n_entries += len(got)
    assert (n_tags, n_entries) == (983, 3217)


# values the grammar rejects, the bit the device must set, and what the host path does with them
REJECTED = [("10,1234567890123456789,+,10M,60,0;", extract.SA_ST_NUMBER, None), ("10,+5,+,10M,60,0;", extract.SA_ST_NUMBER, None),
            ("10,5, 60,10M,60,0;", extract.SA_ST_STRAND, None), ("10,5,+,10S?500M,60,0;", extract.SA_ST_CIGAR, None),
            ("10,5,+,10M, 60,0;", extract.SA_ST_NUMBER, None), ("10,5,+,,60,0;", extract.SA_ST_CIGAR, None), ("10,5,+,M,60,0;", extract.SA_ST_CIGAR, None),
            ("10,5,+,10M5,60,0;", extract.SA_ST_CIGAR, None), ("10,5,+,10M,1234567890,0;", extract.SA_ST_NUMBER, None),
            ("10,5,+,10M;", extract.SA_ST_FIELDS, IndexError), ("9,5,+,10M,60,0;", extract.SA_ST_NAME, KeyError), (";", extract.SA_ST_FIELDS | extract.SA_ST_NAME, IndexError),
            ("10,x,+,10M,60,0;", extract.SA_ST_NUMBER, ValueError), ("10,5,+,10M,60,0;1,,+,10M,60;", extract.SA_ST_NUMBER, ValueError)]
ACCEPTED = ["", "10,5,+,10M,60,0", "10,5,+,10M,60,0;1,7,-,3S4M,2", "10,5,+,*,60,0;", "1,007,x,20H30S100M500N200M10D5I40S10H,000,0,extra,fields;",
            "10,999999999999999999,-,5S,999999999,;"]


def test_strict_grammar_on_values_it_rejects():
    rank = {"1": 1, "10": 0}
    for value, bit, exc in REJECTED:
        assert extract.sa_status(value, rank) == bit, value
        assert strict_parse(value, rank) is None, value
        if exc is None:
            extract.encode_split_reads([([], value, 1000)], rank)              # Python's int() / the regular expression cope: the host path's business
        else:
            with pytest.raises(exc):
                extract.encode_split_reads([([], value, 1000)], rank)
    for value in ACCEPTED:
        assert extract.sa_status(value, rank) == 0, value
        want = extract.encode_split_reads([([], value, 1000)], rank)
        got = strict_parse(value, rank)
        for k, col in enumerate(("c0", "c1", "f0", "f1", "chr", "mapq", "strand")):
            assert [e[k] for e in got] == want[col].tolist(), (value, col)


# ------------------------------------------------------------------------------------------------ GPU
def assert_enc_equal(got, want, where=""):
    for k in ENC_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(5))
def test_gpu_split_inputs_equal_encode_split_reads_on_the_goldens(ctx, tmp_path, which):
    """golden cases: the columns, call_rec and zero flagged calls; then the analysis in place == the analysis on uploaded arrays == the oracle"""
    case, chrom = all_cases()[which]
    p = case["params"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "g.bam")
    bam_writer.write_bam(path, refs, recs)
    ch = one_chunk(path, chrom)
    cols = bam.decode(ctx, ch)
    sel = selection(cols, p["min_read_len"])
    reads, call_rec = old_way(ch, cols, sel, chrom, p["min_mapq"])
    want = extract.encode_split_reads(reads, rank)
    got = extract.split_inputs_bam(ctx, ch, cols, sel, rank, chrom, p["min_mapq"])
    assert got["n_flagged"] == 0 and not got["status"].any()
    assert got["n_calls"] == len(reads) > 50 and got["n_entries"] == int(want["ent_off"][-1]) > 200
    assert_enc_equal(got, want, case["name"])
    assert got["call_rec"].dtype == np.int32 and got["call_rec"].tolist() == call_rec
    assert got["ms_device"] > 0
    # the analysis in place
    a = extract.split_signatures(ctx, None, from_bam=got, **skw(p))
    b = extract.split_signatures(ctx, want, **skw(p))
    o = _oracle().split_signatures(want, **skw(p))
    for k in SPLIT_KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) and np.array_equal(a[k], o[k]), (case["name"], k)
    assert len(a["kind"]) > 20


def _single_pipe_case(ctx, case, path):
    """single_pipe_bam(sa="device") == the recorded reference output, with the region handling of test_bam_reader._single_pipe_bam_case
    (the recorded run saw every record of the case: the region's end is moved behind the last one); on the case's own region == sa="host" """
    p = case["params"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    chrom, t0, t1 = case["task"]
    far = max(t1, max(d["start"] for d in case["reads"]) + 1)
    with bam.BamFile(path) as bf:
        cand, reads_info = extract.single_pipe_bam(ctx, bf, chrom, t0, far, rank, *pipe_args(p), bed_regions=case["bed"], sa="device")
        for t in ("DEL", "INS", "DUP", "INV", "TRA"):
            got = [list(x) for x in cand[t]]
            assert got == case[t], (case["name"], t, len(got), len(case[t]))
        assert [list(x) for x in reads_info] == case["reads_table"] and len(reads_info) > 20
        dev = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, rank, *pipe_args(p), bed_regions=case["bed"], sa="device")
        host = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, rank, *pipe_args(p), bed_regions=case["bed"], sa="host")
        assert dev == host and sum(len(v) for v in dev[0].values()) > 50


@pytest.mark.gpu
def test_gpu_single_pipe_bam_device_sa_equals_the_reference(ctx, tmp_path):
    for case in load_json("single_pipe.json.gz"):
        refs, recs = golden_records(case, case["task"][0])
        path = str(tmp_path / (case["name"] + ".bam"))
        bam_writer.write_bam(path, refs, recs)
        _single_pipe_case(ctx, case, path)
        # no call of the case is flagged: the candidates above came from the device parser
        ch = one_chunk(path, case["task"][0])
        cols = bam.decode(ctx, ch)
        rank = {c: i for i, c in enumerate(case["chroms"])}
        si = extract.split_inputs_bam(ctx, ch, cols, selection(cols, case["params"]["min_read_len"]), rank, case["task"][0], case["params"]["min_mapq"], host_outputs=False)
        assert si["n_flagged"] == 0 and si["n_calls"] > 50 and len(si["c0"]) == 0


# ---- the grammar's edges
EDGE_PARAMS = dict(sv=30, min_mapq=20, parts=-1, min_read_len=500, min_siglength=10, md=0, mi=100, max_size=100000)


def edge_refs():
    """400 contigs, among them "1" and "10" (one name a prefix of the other); ranks REVERSED against the sorted order"""
    names = ["1", "10"] + ["c%03d" % k for k in range(398)]
    rank = {n: len(names) - 1 - i for i, n in enumerate(sorted(names))}
    return [(n, 10 ** 8) for n in names], rank


def edge_records():
    """-> (records on contig "1", names of the records whose calls the device must flag)"""
    long_value = "".join("c%03d,%d,%s,%dS%dM,%d,1;" % (k * 5, 1000 + 977 * k, "+-"[k & 1], 10 * k, 400 + k, 20 + k % 40) for k in range(70))
    assert len(long_value) > 64 * 16 and long_value.count(";") > 64
    ok = "10,5000,+,100S500M50S,60,3;1,9000,-,50S600M,30,1;"
    rows = [("plain", 0, 60, [ok]), ("no_trailing", 16, 60, ["10,5000,+,100S500M,60,3;1,9000,-,50S600M,30,1"]), ("no_semicolon", 0, 60, ["10,5000,+,100S500M,60,3"]),
            ("empty", 0, 60, [""]), ("two_tags", 16, 60, [ok, "c017,77,-,600M100S,60,0;c390,5,+,100S600M,25,0;"]),
            ("secondary", 256, 60, [ok]), ("short", 0, 60, [ok]), ("low_mapq", 0, 5, [ok]), ("star", 0, 60, ["10,5000,+,*,60,3;1,100,+,200S500M,60,0;"]),
            ("hard_and_skip", 16, 60, ["10,5000,-,20H30S100M500N200M10D5I40S10H,60,0;1,20,+,40S100=5X3P,60,0;"]),
            ("flag_19_digits", 0, 60, ["10,1234567890123456789,+,100S500M,60,0;"]), ("flag_plus5", 0, 60, ["10,+5,+,100S500M,60,0;1,900,-,700M,60,0;"]),
            ("flag_regex_skips", 16, 60, ["10,5000,+,100S?500M,60,0;"]), ("flag_strand", 0, 60, ["10,5000,+-,100S500M,60,0;"]),
            ("flag_one_of_two", 0, 60, [ok, "1,900,-,700M, 60,0;"]), ("prefix", 16, 60, ["1,5000,+,100S500M,60,0;10,5000,+,650S500M,60,0;"]),
            ("long", 0, 60, [long_value]), ("extra_fields", 0, 60, ["c397,12,-,100S500M,60,0,x,y,z;"])]
    recs, pos = [], 1000
    for name, flag, mapq, values in rows:
        qlen = 300 if name == "short" else 1150
        recs.append(dict(name=name, flag=flag, mapq=mapq, start=pos, cigar=[(4, 100), (0, qlen - 150), (5, 70)] if name == "hard_and_skip" else [(4, 100), (0, qlen - 150), (4, 50)],
                         seq=synth.pseudo_sequence(qlen - (50 if name == "hard_and_skip" else 0), 31 + len(recs)), refid=0, tags=[("NM", 2)] + [("SA", v) for v in values]))
        pos += 137
    return recs, [n for n, _, _, _ in rows if n.startswith("flag_")]


@pytest.mark.gpu
def test_gpu_grammar_edges(ctx, tmp_path):
    refs, rank = edge_refs()
    recs, must_flag = edge_records()
    p = EDGE_PARAMS
    path = str(tmp_path / "edge.bam")
    bam_writer.write_bam(path, refs, recs)
    ch = one_chunk(path, "1")
    cols = bam.decode(ctx, ch)
    sel = selection(cols, p["min_read_len"])
    assert [ch.name(i) for i in np.flatnonzero(~sel)] == ["secondary", "short"]
    reads, call_rec = old_way(ch, cols, sel, "1", p["min_mapq"])
    got = extract.split_inputs_bam(ctx, ch, cols, sel, rank, "1", p["min_mapq"])
    known = extract.sa_names(rank)
    predicted = [extract.sa_status(v, known) for _, v, _ in reads]
    assert got["status"].tolist() == predicted and got["call_rec"].tolist() == call_rec
    assert sorted({ch.name(call_rec[k]) for k in np.flatnonzero(got["status"])}) == sorted(must_flag) and got["n_flagged"] == len(must_flag)
    assert got["status"][call_rec.index([r["name"] for r in recs].index("flag_one_of_two"))] == 0        # the record's first tag is fine
    # a flagged call has no entries; the others hold exactly what encode_split_reads makes of them
    want = extract.encode_split_reads([r if s == 0 else ([], "", r[2]) for r, s in zip(reads, predicted)], rank)
    assert_enc_equal(got, want)
    low = call_rec.index([r["name"] for r in recs].index("low_mapq"))
    assert got["primary"][got["ent_off"][low]:got["ent_off"][low + 1]].tolist() == [0, 0]               # no primary entry below min_mapq
    # the end result: flagged calls went through the host path, at their place in read order
    with bam.BamFile(path) as bf:
        dev = extract.single_pipe_bam(ctx, bf, "1", 0, 1 << 40, rank, *pipe_args(p), sa="device")
        host = extract.single_pipe_bam(ctx, bf, "1", 0, 1 << 40, rank, *pipe_args(p), sa="host")
    assert dev == host and sum(len(v) for v in dev[0].values()) > 20
    # an entry of four fields, an unknown contig (one that only has a name of the table as its prefix, one that is the prefix of
    # names of the table) and a position that is no number: the device flags them for exactly the predicted reason, and where
    # the host path raises, the device path raises the same
    for value, bit, exc in (("10,5,+,10M;", extract.SA_ST_FIELDS, IndexError), ("nope,5,+,10M,60,0;", extract.SA_ST_NAME, KeyError),
                            ("100,5,+,10M,60,0;", extract.SA_ST_NAME, KeyError), ("c,5,+,10M,60,0;", extract.SA_ST_NAME, KeyError),
                            ("10,x,+,10M,60,0;", extract.SA_ST_NUMBER, ValueError)):
        path2 = str(tmp_path / "raise.bam")
        bam_writer.write_bam(path2, refs, recs[:2] + [dict(recs[0], name="bad", start=5000, tags=[("SA", value)])])
        ch2 = one_chunk(path2, "1")
        cols2 = bam.decode(ctx, ch2)
        sel2 = selection(cols2, p["min_read_len"])
        reads2, _ = old_way(ch2, cols2, sel2, "1", p["min_mapq"])
        st2 = extract.split_inputs_bam(ctx, ch2, cols2, sel2, rank, "1", p["min_mapq"])
        assert st2["status"].tolist() == [extract.sa_status(v, known) for _, v, _ in reads2] == [0, 0, bit], value
        assert st2["n_flagged"] == 1 and st2["ent_off"].tolist() == [0, 3, 5, 5]
        with bam.BamFile(path2) as bf:
            for how in ("host", "device"):
                with pytest.raises(exc):
                    extract.single_pipe_bam(ctx, bf, "1", 0, 1 << 40, rank, *pipe_args(p), sa=how)


@pytest.mark.gpu
def test_gpu_task_to_pool(ctx, tmp_path):
    from cutesv_amd import rebuild
    from cutesv_amd.columns import TYPES
    case = load_json("single_pipe.json.gz")[0]
    p, (chrom, t0, t1) = case["params"], case["task"]
    chroms = case["chroms"]
    rank = {c: i for i, c in enumerate(chroms)}
    n_chrom = len(chroms)
    seg_of = lambda t, ci: TYPES.index(t) * n_chrom + ci                        # noqa: E731
    seg_base = [seg_of(t, 0) for t in ("DEL", "INS", "DUP", "INV", "TRA")]
    seg_ins, seg_del = seg_of("INS", rank[chrom]), seg_of("DEL", rank[chrom])
    major = np.zeros(len(TYPES) * n_chrom, np.uint8); nodedup = np.zeros(len(TYPES) * n_chrom, np.uint8)
    for t in ("INV", "TRA"):
        major[seg_of(t, 0):seg_of(t, 0) + n_chrom] = 1
    nodedup[seg_of("INS", 0):seg_of("INS", 0) + n_chrom] = 1
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "p.bam")
    bam_writer.write_bam(path, refs, recs)
    base = 1000
    with bam.BamFile(path) as bf:
        # ---- the existing path: the CIGAR scan on uploaded arrays + CSV_CG_TO_POOL, split_signatures(enc, pool=...)
        ch = bf.records(chrom, t0, t1)
        cols = bam.decode(ctx, ch)
        n = ch.n
        gate = (cols["cls"] != 0) & (cols["ref_start"] >= t0)
        parsed = gate & (cols["query_len"] >= p["min_read_len"])
        use = (parsed & (cols["mapq"] >= p["min_mapq"])).astype(np.uint8)
        sel = parsed & selection(cols, 0)
        reads, call_rec = old_way(ch, cols, sel, chrom, p["min_mapq"])
        enc = extract.encode_split_reads(reads, rank)
        call_q = [r[2] for r in reads]
        # a row's read index -> the record: records sit at base + i, the calls of the existing path behind them
        to_rec = np.zeros(base + n + len(reads), np.int32)
        to_rec[base:base + n] = np.arange(n); to_rec[base + n:] = call_rec
        rebuild.pool_reset(ctx)
        ckw = dict(min_siglength=p["min_siglength"], merge_ins_threshold=p["mi"], merge_del_threshold=p["md"])
        extract.cigar_signatures(ctx, cols["cig_off"], cols["cigar"], cols["ref_start"], use, pool=dict(seg_ins=seg_ins, seg_del=seg_del, read_base=base, query_len=cols["query_len"]), **ckw)
        n_cigar_rows = rebuild.pool_rows(ctx)
        ssig = extract.split_signatures(ctx, enc, pool=dict(seg_base=seg_base, read_base=base + n, query_len=call_q), **skw(p))
        n_want = rebuild.pool_rows(ctx)
        want = rebuild.rebuild_pool(ctx, to_rec, major, nodedup, keep_on_device=False)
        # ---- CSV_CG_FROM_BAM | CSV_CG_TO_POOL on its own: the same rows as the scan on uploaded arrays
        rebuild.pool_reset(ctx)
        cols2 = bam.decode(ctx, ch, host_outputs=False)
        extract.cigar_signatures(ctx, None, None, None, use, pool=dict(seg_ins=seg_ins, seg_del=seg_del, read_base=base, query_len=cols2["query_len"]),
                                 host_outputs=False, from_bam=cols2, **ckw)
        assert rebuild.pool_rows(ctx) == n_cigar_rows > 50
        # ---- CSV_SP_FROM_BAM | CSV_CG_TO_POOL on its own == pool_rows_of_split with the read mapped from call to record
        rebuild.pool_reset(ctx)
        si = extract.split_inputs_bam(ctx, ch, cols2, sel, rank, chrom, p["min_mapq"], host_outputs=False)
        assert si["n_flagged"] == 0
        extract.split_signatures(ctx, None, from_bam=si, pool=dict(seg_base=seg_base, read_base=base), host_outputs=False, **skw(p))
        rows = extract.pool_rows_of_split(ssig, seg_base, 0, call_q)
        rows["read"] = (base + np.asarray(call_rec, np.int32)[ssig["read"]]).astype(np.int32)
        assert rebuild.pool_rows(ctx) == len(rows["a"]) == n_want - n_cigar_rows > 20
        got_split = rebuild.rebuild_pool(ctx, to_rec, major, nodedup, keep_on_device=False)
        want_split = rebuild.rebuild_columns(ctx, rows["seg"], rows["a"], rows["b"], to_rec[rows["read"]], rows["aux"], major, nodedup)
        for k in ("seg_id", "a", "b", "read_id", "aux", "src_row"):
            assert np.array_equal(got_split[k], want_split[k]), k
        # ---- task_to_pool: one call from the file's region to the pool
        rebuild.pool_reset(ctx)
        res = extract.task_to_pool(ctx, bf, chrom, t0, t1, rank, *pipe_args(p), seg_ins, seg_del, seg_base, base, bed_regions=case["bed"])
        assert rebuild.pool_rows(ctx) == n_want
        got = rebuild.rebuild_pool(ctx, to_rec, major, nodedup, keep_on_device=False)
        for k in ("seg_id", "a", "b", "read_id", "aux", "src_row"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["seg_count"], want["seg_count"])
        assert res["n_flagged"] == 0 and len(res["flagged_calls"]) == 0 and res["n_records"] == n and res["n_calls"] == len(reads)
        assert res["n_sig_ins"] + res["n_sig_del"] == n_cigar_rows and res["n_split"] == n_want - n_cigar_rows and res["n_split_host"] == 0
        # the reads table, as columns
        _, reads_info = extract.single_pipe_bam(ctx, bf, chrom, t0, t1, rank, *pipe_args(p), bed_regions=case["bed"])
        table = list(zip(res["reads_start"].tolist(), res["reads_end"].tolist(), res["reads_primary"].tolist(), [ch.name(i) for i in res["reads_index"].tolist()],
                         [chrom] * len(res["reads_index"])))
        assert table == reads_info and len(table) > 10
    rebuild.pool_reset(ctx)


@pytest.mark.gpu
def test_gpu_task_to_pool_appends_the_rows_of_flagged_calls(ctx, tmp_path):
    """the edge file through task_to_pool: the pool holds the rows of single_pipe's split candidates, flagged calls included"""
    from cutesv_amd import rebuild
    refs, rank = edge_refs()
    recs, must_flag = edge_records()
    p = EDGE_PARAMS
    path = str(tmp_path / "edge.bam")
    bam_writer.write_bam(path, refs, recs)
    n_chrom = len(rank)
    seg_base = [k * n_chrom for k in range(5)]
    rebuild.pool_reset(ctx)
    with bam.BamFile(path) as bf:
        res = extract.task_to_pool(ctx, bf, "1", 0, 1 << 40, rank, *pipe_args(p), 5 * n_chrom, 5 * n_chrom + 1, seg_base, 0)
        ch = bf.records("1", 0, 1 << 40)
    assert sorted({ch.name(i) for i in res["flagged_records"].tolist()}) == sorted(must_flag) and res["n_flagged"] == len(must_flag)
    cols = bam.decode_host(ch)
    sel = selection(cols, p["min_read_len"])
    reads, call_rec = old_way(ch, cols, sel, "1", p["min_mapq"])
    ssig = extract.split_signatures(ctx, extract.encode_split_reads(reads, rank), **skw(p))
    assert res["n_split"] + res["n_split_host"] == len(ssig["kind"]) and res["n_split_host"] > 0
    assert rebuild.pool_rows(ctx) == len(ssig["kind"]) + res["n_sig_ins"] + res["n_sig_del"]
    rows = extract.pool_rows_of_split(ssig, seg_base, 0, [r[2] for r in reads])
    rows["read"] = np.asarray(call_rec, np.int32)[ssig["read"]]
    ident = np.arange(ch.n, dtype=np.int32)
    zeros = np.zeros(5 * n_chrom + 2, np.uint8)
    got = rebuild.rebuild_pool(ctx, ident, zeros, zeros, keep_on_device=False)
    want = rebuild.rebuild_columns(ctx, rows["seg"], rows["a"], rows["b"], rows["read"], rows["aux"], zeros, zeros)
    for k in ("seg_id", "a", "b", "read_id", "aux"):
        assert np.array_equal(got[k], want[k]), k
    rebuild.pool_reset(ctx)


def device_memory_free():
    """free bytes of the current device, asked of the HIP runtime the library itself is linked with"""
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "the HIP runtime library was not found"
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


@pytest.mark.gpu
def test_gpu_pool_only_calls_keep_the_arena_small(tmp_path):
    """The candidate columns of csv_split_signatures are sized by what the entries can yield (12 per entry), not by the capacity
    the caller names: task_to_pool - which asks for no host arrays - and a direct call with a capacity of 2^31 and NULL arrays
    leave the context's device memory within 8 GiB of where it was (a capacity taken at its word would be ~100 GB).  The bound
    is wide because other processes share the card."""
    from cutesv_amd import engine, rebuild
    case = load_json("single_pipe.json.gz")[0]
    p, (chrom, t0, t1) = case["params"], case["task"]
    rank = {c: i for i, c in enumerate(case["chroms"])}
    refs, recs = golden_records(case, chrom)
    path = str(tmp_path / "a.bam")
    bam_writer.write_bam(path, refs, recs)
    with engine.Context(0) as c2, bam.BamFile(path) as bf:
        ch = bf.records(chrom, t0, 1 << 40)
        bam.decode(c2, ch, host_outputs=False)                # (the context's first allocations are behind it)
        before = device_memory_free()
        res = extract.task_to_pool(c2, bf, chrom, t0, 1 << 40, rank, *pipe_args(p), 5, 0, [0, 5, 10, 15, 20], 0)
        assert res["n_split"] > 50 and res["n_flagged"] == 0
        after_task = device_memory_free()
        cols = bam.decode(c2, ch, host_outputs=False)
        si = extract.split_inputs_bam(c2, ch, cols, selection(cols, p["min_read_len"]), rank, chrom, p["min_mapq"], host_outputs=False)
        L = _lib.lib()
        sin = extract.SplitIn(sv_size=p["sv"], max_size=p["max_size"], min_mapq=p["min_mapq"], max_split_parts=p["parts"], flags=_abi.SP_FROM_BAM | _abi.CG_TO_POOL)
        sin.pool_seg_base = (C.c_int32 * 5)(0, 5, 10, 15, 20)
        sout = extract.SplitOut(cap=(1 << 31) - 8192)
        assert L.csv_split_signatures(c2._h, C.byref(sin), C.byref(sout)) == _abi.OK and 50 < sout.n <= 12 * si["n_entries"]
        after_call = device_memory_free()
        rebuild.pool_reset(c2)
    assert before - after_task < 8 << 30 and before - after_call < 8 << 30, (before, after_task, after_call)


@pytest.mark.gpu
def test_gpu_split_inputs_misuse(tmp_path):
    from cutesv_amd import engine
    from cutesv_amd.engine import CsvError
    case = load_json("single_pipe.json.gz")[0]
    refs, recs = golden_records(case, "7")
    path = str(tmp_path / "m.bam")
    bam_writer.write_bam(path, refs, recs[:60])
    ch = one_chunk(path, "7")
    rank = {c: i for i, c in enumerate(case["chroms"])}
    with engine.Context(0) as c2:
        host_cols = bam.decode_host(ch)
        sel = selection(host_cols, 0)
        with pytest.raises(CsvError) as e:                  # no decode in the context
            extract.split_inputs_bam(c2, ch, host_cols, sel, rank, "7", 20)
        assert e.value.code == _abi.E_INVALID
        with pytest.raises(CsvError) as e:                  # CSV_SP_FROM_BAM without split inputs
            extract.split_signatures(c2, None, from_bam=dict(n_calls=3))
        assert e.value.code == _abi.E_INVALID
        cols = bam.decode(c2, ch)
        with pytest.raises(CsvError) as e:                  # decoded, but still no split inputs
            extract.split_signatures(c2, None, from_bam=dict(n_calls=3))
        assert e.value.code == _abi.E_INVALID

        class Short:
            n = ch.n - 1
        with pytest.raises(CsvError) as e:                  # a record count that is not the decode's
            extract.split_inputs_bam(c2, Short, cols, sel[:-1], rank, "7", 20)
        assert e.value.code == _abi.E_INVALID
        # a name table that is not sorted: straight through the C entry
        L = _lib.lib()
        sel8 = np.ascontiguousarray(sel, np.uint8)
        for blob, off in ((b"101", [0, 2, 3]), (b"11", [0, 1, 2]), (b"110", [0, 1, 4]), (b"110", [0, 2, 1])):
            names = np.frombuffer(blob, np.uint8); name_off = np.asarray(off, np.int64); name_rank = np.zeros(2, np.int32)
            sin = extract.SaIn(n_records=ch.n, sel=sel8.ctypes.data, min_mapq=20, task_rank=0, n_names=2, names=names.ctypes.data, name_bytes=len(blob),
                               name_off=name_off.ctypes.data, name_rank=name_rank.ctypes.data)
            sout = extract.SaOut()
            assert L.csv_bam_split_inputs(c2._h, C.byref(sin), C.byref(sout)) == _abi.E_INVALID, (blob, off)
        # ... and the context still works
        got = extract.split_inputs_bam(c2, ch, cols, sel, rank, "7", 20)
        assert got["n_calls"] > 5 and got["n_flagged"] == 0
        # a new decode drops the split inputs
        bam.decode(c2, ch, host_outputs=False)
        with pytest.raises(CsvError):
            extract.split_signatures(c2, None, from_bam=got)
