"""The SA-tag parser (sa.hip.h) at its seams: the 16-byte block a lane reads, the 1 KiB step of a wavefront, the 64 entries of a
round, the spans of the one-workgroup scans.

The truth is extract.encode_split_reads on the calls built the old way, plus extract.sa_status for the calls the device must
flag - as test_bam_split.test_gpu_grammar_edges compares.  Every crafted record says where its value lies in the slim image (start
and end residue mod 16, the byte a ';' sits on, the length from the 16-byte floor of its start) and the test asserts that claim on
the decoded sa_beg / sa_end before it compares anything: a case that missed its seam fails, it does not pass vacuously.
Values are padded with digits in the sixth field (NM), which neither side parses."""
import numpy as np
import pytest

from cutesv_amd import bam, extract, synth
import bam_writer
from test_bam_split import (old_way, selection, strict_parse, assert_enc_equal, one_chunk, edge_refs, pipe_args, EDGE_PARAMS)

NUMBER, STRAND, CIGAR, FIELDS, NAME = extract.SA_ST_NUMBER, extract.SA_ST_STRAND, extract.SA_ST_CIGAR, extract.SA_ST_FIELDS, extract.SA_ST_NAME
P = EDGE_PARAMS
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 193)
BAD_AT = (0, 63, 64, 65, 128)
BAD = (("four_fields", "c001,5,+,10M;", FIELDS, True), ("plus5", "c001,+5,+,10M,60,0;", NUMBER, False), ("unknown", "zzz,5,+,10M,60,0;", NAME, True))
D18 = "9" * 18


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def ent(k, nm="0"):
    """entry k: every number is its own, so an entry read from a wrong slot shows"""
    return "c%03d,%d,%s,%dS%dM,%d,%s;" % (k % 398, 1000 + 977 * k, "+-"[k & 1], 10 * k + 1, 400 + k, 20 + k % 40, nm)


def ents(n, first=0):
    return [ent(first + k) for k in range(n)]


def pad(entries, idx, extra):
    """`extra` more digits in the NM field of entry idx"""
    assert extra >= 0 and entries[idx].endswith(";")
    out = list(entries)
    out[idx] = out[idx][:-1] + "7" * extra + ";"
    return out


def crafted():
    """-> [dict(name, values, res (start of the FIRST value mod 16), flag, mapq, cigar, bits (per value), raises, claims)]"""
    rows = []

    def add(name, values, res=5, flag=0, mapq=60, cigar=None, bits=None, raises=False, **claims):
        rows.append(dict(name=name, values=values, res=res, flag=flag, mapq=mapq, cigar=cigar, bits=bits or [0] * len(values), raises=raises, claims=claims))

    three = ents(3, 7)
    for r in range(16):                                      # the value's start on every residue, then its end
        add("start_%02d" % r, ["".join(three)], res=r, start_res=r)
    for r in range(16):
        v = "".join(three)
        add("end_%02d" % r, ["".join(pad(three, 1, (r - 3 - len(v)) % 16))], res=3, end_res=r)
    for n in COUNTS:                                         # entries per value around the 64 of a round
        v = "".join(ents(n, 3)) if n else ent(3)[:-1]
        add("count_%03d" % n, [v], res=(3 * n) % 16, n_semi=n)
    for k, r in ((0, 15), (0, 0), (1, 15), (1, 0), (2, 15), (2, 0)):   # a ';' on the last / first byte of a 16-byte block
        e = ents(4, 11)
        at = len("".join(e[:k + 1])) - 1                     # offset of entry k's ';' in the value
        add("semi_%d_on_%02d" % (k, r), ["".join(pad(e, k, (r - 9 - at) % 16))], res=9, semi_at=(k, r))
    for total in (1023, 1024, 1025, 2047, 2048, 2049):       # the length from the 16-byte floor of the start: around one and two steps
        e = ents(total // 40, 5)
        add("floor_len_%d" % total, ["".join(pad(e, len(e) - 1, total - 6 - len("".join(e))))], res=6, floor_len=total)
    for off in (1023, 1024, 2047):                           # a ';' on that byte from the floor: the next entry begins on the next step's first byte
        e = ents(80, 9)
        k = max(j for j in range(len(e)) if len("".join(e[:j + 1])) - 1 + 4 <= off)
        at = len("".join(e[:k + 1])) - 1
        add("semi_on_byte_%d" % off, ["".join(pad(e, k, off - 4 - at))], res=4, semi_off=off)
    for what, text, bit, raises in BAD:                      # one bad entry behind the first round
        for at in BAD_AT:
            e = ents(130, 2)
            e[at] = text
            add("bad_%s_%03d" % (what, at), ["".join(ents(2, 40)), "".join(e), "".join(ents(3, 50))], res=(at + bit) % 16, bits=[0, bit, 0], raises=raises)
    e = ents(4, 13)
    add("empty_entry", ["".join(e[:2]) + ";" + "".join(e[2:])], bits=[FIELDS | NAME], raises=True)
    add("trailing_text", ["".join(e) + "c001,5,+,10"], n_semi=4)
    add("trailing_garbage", ["".join(e) + ",,,?"], n_semi=4)
    # number widths (a number beyond 64 / 32 bits overflows the host path's columns: those records stay out of the end-to-end comparison)
    add("pos_18", ["10,%s,+,100S500M,60,0;" % D18])
    add("pos_19", ["10,%s9,+,100S500M,60,0;" % D18], bits=[NUMBER], raises=True)
    add("mapq_9", ["10,5000,+,100S500M,%s,0;" % ("9" * 9)])
    add("mapq_10", ["10,5000,+,100S500M,%s,0;" % ("9" * 10)], bits=[NUMBER], raises=True)
    add("cigar_18", ["10,5000,+,%sS500M,60,0;" % D18])
    add("cigar_19", ["10,5000,+,%s9S500M,60,0;" % D18], bits=[CIGAR], raises=True)
    add("span_4", ["10,5000,+,%s,60,0;" % ((D18 + "M") * 4)])
    add("span_5", ["10,5000,+,%s,60,0;" % ((D18 + "M") * 5)], bits=[CIGAR])
    add("single_S", ["10,5000,+,100S,60,0;1,77,-,100M,60,0;"])
    # the primary entry
    add("mapq_below", ["".join(three)], mapq=P["min_mapq"] - 1, n_primary=0)
    add("mapq_at", ["".join(three)], mapq=P["min_mapq"], n_primary=1)
    add("fwd_clips", ["".join(three)], flag=0, n_primary=1)
    add("rev_clips", ["".join(three)], flag=16, n_primary=1)
    add("left_H_fwd", ["".join(three)], flag=0, cigar=[(5, 70), (0, 1030), (4, 50)], n_primary=1)
    add("left_H_rev", ["".join(three)], flag=16, cigar=[(5, 70), (0, 1030), (4, 50)], n_primary=1)
    return rows


def records(rows):
    """the crafted rows as BAM records on contig "1": the first value starts on residue `res` of the slim image.  A record's image is
    32 fixed bytes, 4 per operation, then the tags: XZ:Z:<c characters>\\0 (4 + c bytes), then S A Z (3 bytes) and the value."""
    recs, pos = [], 1000
    for k, row in enumerate(rows):
        cig = row["cigar"]
        if cig is None:
            extra = k % 4                                    # the operation count mod 4 moves the start in steps of 4 bytes
            cig = [(4, 100)] + [(0, 250)] * 3 + [(7, 250)] + [(8, 1)] * extra + [(4, 50)]
            cig[1] = (0, 250 - extra)
        c = (row["res"] - 7 - 4 * len(cig)) % 16
        qlen = sum(ln for op, ln in cig if op in (0, 1, 4, 7, 8))
        recs.append(dict(name=row["name"], flag=row["flag"], mapq=row["mapq"], start=pos, cigar=cig, seq=synth.pseudo_sequence(qlen, 500 + k), refid=0,
                         tags=[("XZ", "Z", "x" * c)] + [("SA", v) for v in row["values"]]))
        pos += 137
    return recs


def assert_geometry(rows, chunk, cols):
    """every case lies in the image where it claims to"""
    slim = np.asarray(chunk.slim)
    seen = set()
    for i, row in enumerate(rows):
        t = int(cols["sa_off"][i])
        assert int(cols["sa_off"][i + 1]) - t == len(row["values"]), row["name"]
        beg, end = int(cols["sa_beg"][t]), int(cols["sa_end"][t])
        value = row["values"][0]
        assert end - beg == len(value) and bytes(slim[beg:end]).decode() == value, row["name"]
        assert beg % 16 == row["res"], (row["name"], beg % 16)
        base = beg & ~15
        semis = [beg + j for j, ch in enumerate(value) if ch == ";"]
        for key, v in row["claims"].items():
            seen.add(key)
            if key == "start_res":
                assert beg % 16 == v
            elif key == "end_res":
                assert end % 16 == v, (row["name"], end % 16)
            elif key == "n_semi":
                assert len(semis) == v
            elif key == "semi_at":
                assert semis[v[0]] % 16 == v[1], (row["name"], semis[v[0]] % 16)
            elif key == "floor_len":
                assert end - base == v, (row["name"], end - base)
            elif key == "semi_off":
                assert base + v in semis and slim[base + v] == ord(";") and base + v + 1 < end, row["name"]
    assert seen == {"start_res", "end_res", "n_semi", "semi_at", "floor_len", "semi_off", "n_primary"}


def test_the_crafted_records_cover_what_they_claim():
    rows = crafted()
    assert {r["claims"].get("start_res") for r in rows} >= set(range(16)) and {r["claims"].get("end_res") for r in rows} >= set(range(16))
    assert {r["claims"]["n_semi"] for r in rows if "n_semi" in r["claims"]} >= set(COUNTS)
    assert len({r["name"] for r in rows}) == len(rows)
    assert len({len(r["cigar"]) % 4 for r in records(rows)}) == 4


def test_geometry_of_the_crafted_records_on_the_host_decode(tmp_path):
    refs, rank = edge_refs()
    rows = crafted()
    path = str(tmp_path / "seams.bam")
    bam_writer.write_bam(path, refs, records(rows))
    ch = one_chunk(path, "1")
    cols = bam.decode_host(ch)
    assert_geometry(rows, ch, cols)
    sel = selection(cols, P["min_read_len"])
    assert sel.all()
    reads, _ = old_way(ch, cols, sel, "1", P["min_mapq"])
    assert [v for _, v, _ in reads] == [v for row in rows for v in row["values"]]


def test_strict_grammar_agrees_with_encode_split_reads_on_every_crafted_value():
    _, rank = edge_refs()
    known = extract.sa_names(rank)
    n = 0
    for row in crafted():
        for value, bits in zip(row["values"], row["bits"]):
            assert extract.sa_status(value, known) == bits, row["name"]
            got = strict_parse(value, rank)
            if bits:
                assert got is None, row["name"]
                continue
            want = extract.encode_split_reads([([], value, 1000)], rank)
            assert got is not None and len(got) == int(want["ent_off"][-1]) == value.count(";"), row["name"]
            for k, col in enumerate(("c0", "c1", "f0", "f1", "chr", "mapq", "strand")):
                assert [e[k] for e in got] == want[col].tolist(), (row["name"], col)
            n += len(got)
    assert n > 1400
    want = extract.encode_split_reads([([], "10,5000,+,100S,60,0;", 1000)], rank)
    assert want["c0"].tolist() == want["c1"].tolist() == [100] and want["f1"].tolist() == [0]
    assert extract.encode_split_reads([([], "10,5,+,%s,60,0;" % ((D18 + "M") * 4), 1000)], rank)["f1"].tolist() == [4 * (10 ** 18 - 1)]


# ------------------------------------------------------------------------------------------------ GPU
def compare(ctx, chunk, cols, rank, min_read_len, where):
    """split_inputs_bam == encode_split_reads on the calls built the old way (a flagged call: no entries) -> (device result, calls, predicted status)"""
    sel = selection(cols, min_read_len)
    reads, call_rec = old_way(chunk, cols, sel, "1", P["min_mapq"])
    got = extract.split_inputs_bam(ctx, chunk, cols, sel, rank, "1", P["min_mapq"])
    known = extract.sa_names(rank)
    predicted = [extract.sa_status(v, known) for _, v, _ in reads]
    assert got["status"].tolist() == predicted, where
    assert got["call_rec"].tolist() == call_rec and got["n_calls"] == len(reads) and got["n_flagged"] == sum(1 for s in predicted if s), where
    want = extract.encode_split_reads([r if s == 0 else ([], "", r[2]) for r, s in zip(reads, predicted)], rank)
    assert_enc_equal(got, want, where)
    assert got["n_entries"] == int(want["ent_off"][-1])
    return got, reads, call_rec, predicted


@pytest.mark.gpu
def test_gpu_crafted_values_equal_encode_split_reads(ctx, tmp_path):
    refs, rank = edge_refs()
    rows = crafted()
    recs = records(rows)
    path = str(tmp_path / "seams.bam")
    bam_writer.write_bam(path, refs, recs)
    ch = one_chunk(path, "1")
    cols = bam.decode(ctx, ch)
    assert_geometry(rows, ch, cols)
    got, reads, call_rec, predicted = compare(ctx, ch, cols, rank, P["min_read_len"], "seams")
    assert predicted == [b for row in rows for b in row["bits"]]
    # a flagged call has no entries and the calls around it keep theirs
    first_call = np.concatenate([[0], np.cumsum([len(r["values"]) for r in rows])])
    n_ent = np.diff(got["ent_off"])
    for i, row in enumerate(rows):
        k = int(first_call[i])
        if row["name"].startswith("bad_"):
            assert n_ent[k:k + 3].tolist() == [3, 0, 4], row["name"]
        if "n_primary" in row["claims"]:
            a, b = int(got["ent_off"][k]), int(got["ent_off"][k + 1])
            assert int(got["primary"][a:b].sum()) == row["claims"]["n_primary"] and b - a == 3 + row["claims"]["n_primary"], row["name"]
            if row["claims"]["n_primary"]:
                cig = recs[i]["cigar"]
                left, right, ql = cig[0][1], cig[-1][1], int(cols["query_len"][i])
                fwd = row["flag"] == 0
                assert (int(got["c0"][a]), int(got["c1"][a]), int(got["strand"][a])) == ((left, ql - right, 0) if fwd else (right, ql - left, 1)), row["name"]
                assert left != right
        if row["name"] == "single_S":
            a = int(got["ent_off"][k]) + 1
            assert got["c0"][a] == got["c1"][a] == 100 and got["f1"][a] == 0
    # the end result: the same candidates whether the device or the host parses (the values whose host path raises are left out)
    keep = [r for r, row in zip(recs, rows) if not row["raises"]]
    path2 = str(tmp_path / "seams_ok.bam")
    bam_writer.write_bam(path2, refs, keep)
    with bam.BamFile(path2) as bf:
        dev = extract.single_pipe_bam(ctx, bf, "1", 0, 1 << 40, rank, *pipe_args(P), sa="device")
        host = extract.single_pipe_bam(ctx, bf, "1", 0, 1 << 40, rank, *pipe_args(P), sa="host")
    assert dev == host and sum(len(v) for v in dev[0].values()) > 100


def span_records(n=2049):
    """record i: i mod 4 SA tags of 1..3 entries each; every seventh record is too short to be selected, some are secondary"""
    recs, k = [], 0
    for i in range(n):
        short, flag = i % 7 == 3, 256 if i % 11 == 5 else 16 if i % 2 else 0
        ql = 40 if short else 60
        tags = []
        for t in range(i % 4):
            tags.append(("SA", "".join(ents(1 + (i + t) % 3, k))))
            k += 3
        recs.append(dict(name="s%04d" % i, flag=flag, mapq=19 + i % 3, start=1000 + 3 * i, cigar=[(4, 5), (0, ql - 15), (4, 10)], seq=synth.pseudo_sequence(ql, 9000 + i), refid=0, tags=tags))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_records,per_records,per_calls", ((4096, 3, 3), (1500, 2, 2)))
def test_gpu_scan_spans_of_two_and_three(ctx, tmp_path, chunk_records, per_records, per_calls):
    """more than 1 024 records and more than 1 024 calls: every thread of the one-workgroup scans owns a span of 2 or 3"""
    refs, rank = edge_refs()
    recs = span_records()
    path = str(tmp_path / "span.bam")
    bam_writer.write_bam(path, refs, recs)
    with bam.BamFile(path) as bf:
        ch = next(iter(bf.chunks("1", chunk_records=chunk_records)))
    assert ch.n == min(chunk_records, 2049)
    cols = bam.decode(ctx, ch)
    host = bam.decode_host(ch)
    assert np.array_equal(cols["sa_off"], host["sa_off"]) and np.array_equal(cols["cig_off"], host["cig_off"])
    got, reads, call_rec, predicted = compare(ctx, ch, cols, rank, 50, "span")
    assert not any(predicted)
    assert (ch.n + 1023) // 1024 == per_records and (got["n_calls"] + 1023) // 1024 == per_calls
    sel = selection(cols, 50)
    assert 0 < int((~sel & (np.diff(cols["sa_off"]) > 0)).sum()) and got["n_entries"] > got["n_calls"] > 1024
