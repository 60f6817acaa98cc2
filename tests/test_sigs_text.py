"""The text signature files of cuteSV's --write_old_sigs, made on the device from a kept pool rebuild (csv_pool_sigs_text,
kernels in cutesv_amd/csrc/vcf_strings.hip.h; rebuild.sigs_text / sigs_text_host / write_sigs).

CPU: the interface, and the host twin against the files the reference's process_process_sigs_type wrote (golden/old_sigs.json.gz)
byte for byte, with every refusal of the contract.  GPU: the kernels against the twin on a crafted pool (digit counts, name and
sequence lengths around the 64-lane and 4-byte steps, row ranges around the scan tile), the golden cases through the device route,
capacity and misuse, and call_bam(sigs_dir=...) on the planted BAM."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, call, extract, rebuild
from cutesv_amd.columns import Params, SigStore, TYPES
from helpers import load_json, rebuild_case_inputs
import call_helpers
import sigs_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def golden_cases():
    """[(name, the candidates as rebuild_case_inputs gives them, the reference's sorted lists, {TYPE: text of TYPE.sigs})]"""
    by_name = {c["name"]: c for c in load_json("rebuild_order.json.gz")}
    out = []
    for g in load_json("old_sigs.json.gz"):
        case = g if "files" in g else by_name[g["name"]]
        out.append((g["name"], rebuild_case_inputs(case)[0], case["out"], g["sigs"]))
    return out


def case_chroms(per):
    return sorted({x[-1] for t in per for x in per[t]} | {x[2] for x in per["TRA"]})


# ------------------------------------------------------------------------------------------------ CPU: the interface
def test_header_declares_and_lib_binds_the_entry():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    assert re.search(r"^#define CSV_ABI_VERSION 9$", header, re.M)
    m = re.search(r"^int csv_pool_sigs_text\(([^;]*)\);", header, re.M | re.S)
    assert m
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    res, args = bound["csv_pool_sigs_text"]
    assert res is C.c_int and len(args) == m.group(1).count(",") + 1            # one ctypes argument per declared parameter
    L = _lib.lib()
    assert L.csv_abi_version() == _abi.ABI_VERSION == 9
    need = C.c_int64(-1)
    assert L.csv_pool_sigs_text(None, 0, 0, b"", None, 1, b"++", b"--", None, 0, C.byref(need), None) == _abi.E_INVALID
    assert os.path.exists(os.path.join(ROOT, "cutesv_amd", "csrc", "stage_sigs_text.hip.h"))


# ------------------------------------------------------------------------------------------------ CPU: the host twin
def _store_columns(st):
    """a SigStore's rows as the rebuild's columns: seg_id from its segment index, src_row = the row itself (ins_seq is keyed by it)"""
    n_chrom = len(st.chroms)
    seg = np.full(st.n_sig, -1, np.int64)
    for (t, ch), (b, e) in st.seg_index.items():
        seg[b:e] = TYPES.index(t) * n_chrom + st.chroms.index(ch)
    return dict(seg_id=seg, a=st.a, b=st.b, read_id=st.read_id, aux=st.aux, src_row=np.arange(st.n_sig))


def test_host_twin_writes_the_references_files():
    n_lines = 0
    for name, _, out, sigs in golden_cases():
        lists = {t: [tuple(x) for _, rows in out[t] for x in rows] for t in TYPES}
        st = SigStore.from_tuple_lists(lists, chroms=case_chroms(lists))
        cols = _store_columns(st)
        first = np.arange(len(st.names))
        assert st.strands == ("++", "--")
        ranges = rebuild.type_row_ranges([st.seg_index.get((t, c), (0, 0))[1] - st.seg_index.get((t, c), (0, 0))[0] for t in TYPES for c in st.chroms], len(st.chroms))
        for t in TYPES:
            got = rebuild.sigs_text_host(cols, st.names.names, first, st.ins_seq, st.chroms, *ranges[t])
            assert got == sigs[t].encode(), (name, t)
            n_lines += got.count(b"\n")
        whole = rebuild.sigs_text_host(cols, st.names.names, first, st.ins_seq, st.chroms, 0, st.n_sig)
        assert whole == "".join(sigs[t] for t in TYPES).encode(), name
        assert rebuild.sigs_text_host(cols, st.names.names, first, st.ins_seq, st.chroms, 5, 5) == b""
    assert n_lines > 3000
    crafted = [g for g in golden_cases() if g[0] == "crafted"][0][3]
    assert "INS\tchr2\t100\t40\treadB\t" in crafted["INS"] and crafted["INS"].count("\ttie\t") == 3 and crafted["INS"].count("readA") == 1
    assert {ln.split("\t")[2] + ln.split("\t")[4] for ln in crafted["TRA"].splitlines()} >= {k + m for k in "ABCD" for m in ("chr2", "chr10")}
    assert "\t++\t" in crafted["INV"] and "\t--\t" in crafted["INV"]


def test_host_twin_refuses_what_the_entry_refuses():
    chroms = ["c0", "c1"]
    names, first, seqs = ["r0", "r1"], [0, 1], {1: "ACGT"}

    def text(**over):
        row = dict(seg_id=[0], a=[5], b=[6], read_id=[1], aux=[0], src_row=[0])
        row.update(over)
        return rebuild.sigs_text_host(row, names, first, seqs, chroms, 0, 1)
    assert text() == b"DEL\tc0\t5\t6\tr1\n"
    assert text(seg_id=[3], aux=[4], src_row=[1]) == b"INS\tc1\t5\t6\tr1\tACGT\n"
    assert text(seg_id=[4], aux=[1]) == b"INV\tc0\t--\t5\t6\tr1\n"
    assert text(seg_id=[9], aux=[0 * 8 + 3]) == b"TRA\tc1\tD\t5\tc0\t6\tr1\n"
    assert text(a=[(1 << 42) - 1]) == b"DEL\tc0\t4398046511103\t6\tr1\n"
    for bad in (dict(a=[-1]), dict(b=[-1]), dict(a=[1 << 42]), dict(b=[1 << 42]), dict(read_id=[2]), dict(read_id=[-1]),
                dict(seg_id=[2], aux=[4], src_row=[0]),            # an INS row without a sequence
                dict(seg_id=[8], aux=[5]), dict(seg_id=[8], aux=[2 * 8 + 1]),      # TRA: type 5, chr2 = n_chrom
                dict(seg_id=[4], aux=[2]), dict(seg_id=[10]), dict(seg_id=[-1])):
        with pytest.raises(ValueError):
            text(**bad)
    for r0, r1 in ((0, 2), (-1, 1), (1, 0)):
        with pytest.raises(ValueError):
            rebuild.sigs_text_host(dict(seg_id=[0], a=[5], b=[6], read_id=[1], aux=[0], src_row=[0]), names, first, seqs, chroms, r0, r1)


# ------------------------------------------------------------------------------------------------ GPU: the kernels against the twin
VALUES = (0, 9, 10, 99_999, 10 ** 9, (1 << 31) - 1, 1 << 31, (1 << 42) - 1)
NAME_LENS = (1, 63, 64, 65, 255)
SEQ_LENS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)
CRAFTED_CHROMS = ["1", "c" * 40, "chrM"]                  # (sorted: index = name rank)


def crafted_rows(seed=11, n=2300):
    """rows of every type over three contigs: every value of VALUES in both number columns, names and sequences of the lengths
    above, TRA rows of all four types to a mate other than their own contig, both strands, and no DEL row on the middle contig"""
    rng = np.random.default_rng(seed)
    pool_names = [("%c" % (65 + k)) * ln for k, ln in enumerate(NAME_LENS)] + ["read/%d" % k for k in range(40)]
    r = dict(seg=[], a=[], b=[], aux=[], names=[], seqs={}, halves={})
    for k in range(n):
        ti, ch = k % 5, int(rng.integers(0, 3))
        t = TYPES[ti]
        if t == "DEL" and ch == 1:
            ch = 2 * int(rng.integers(0, 2))
        aux = 0
        if t == "INS":
            ln = SEQ_LENS[(k // 5) % len(SEQ_LENS)]
            r["seqs"][k] = "".join("ACGTN"[i] for i in rng.integers(0, 5, ln))
            r["halves"][k] = int(rng.integers(0, 2))
            aux = ln
        elif t == "INV":
            aux = int(rng.integers(0, 2))
        elif t == "TRA":
            aux = ((ch + 1 + int(rng.integers(0, 2))) % 3) * 8 + (k // 5) % 4
        r["seg"].append(ti * 3 + ch); r["aux"].append(aux)
        r["a"].append(VALUES[int(rng.integers(0, len(VALUES)))]); r["b"].append(VALUES[int(rng.integers(0, len(VALUES)))])
        r["names"].append(pool_names[int(rng.integers(0, len(pool_names)))].encode())
    return r


@pytest.fixture(scope="module")
def crafted(ctx):
    """the crafted pool with its kept rebuild, the same rebuild on the host, and the twin's lines: shared, never changed"""
    rows = crafted_rows()
    sigs_helpers.fill_pools(ctx, rows)
    host, first = sigs_helpers.host_rebuild(ctx, 3)
    rb = sigs_helpers.kept_rebuild(ctx, 3)
    assert np.array_equal(rb["src_row"], host["src_row"]) and rb["n_out"] == len(host["a"])
    whole = rebuild.sigs_text_host(host, rows["names"], first, rows["seqs"], CRAFTED_CHROMS, 0, rb["n_out"])
    return rows, host, first, rb, whole.splitlines(keepends=True)


@pytest.mark.gpu
def test_gpu_sigs_text_is_the_twin_on_the_crafted_pool(ctx, crafted):
    rows, host, first, rb, lines = crafted
    sigs_helpers.fill_pools(ctx, rows)                      # (another test of this file may have used the context since the fixture ran)
    rb = sigs_helpers.kept_rebuild(ctx, 3)
    n = rb["n_out"]
    assert n >= 2050 and len(lines) == n and np.array_equal(rb["src_row"], host["src_row"])
    # what the pool was crafted to hold did reach the rebuild
    seg = host["seg_id"]
    assert set((seg // 3).tolist()) == {0, 1, 2, 3, 4}
    cnt = rb["seg_count"]
    assert cnt[0] > 0 and cnt[1] == 0 and cnt[2] > 0                                   # an empty segment between two full ones
    assert set(host["a"].tolist()) == set(VALUES) and set(host["b"].tolist()) == set(VALUES)
    used = {len(rows["names"][i]) for i in first[host["read_id"]].tolist()}
    assert set(NAME_LENS) <= used
    ins = seg // 3 == 1
    assert set(host["aux"][ins].tolist()) == set(SEQ_LENS)
    tra = seg // 3 == 4
    assert set((host["aux"][tra] & 7).tolist()) == {0, 1, 2, 3} and ((host["aux"][tra] >> 3) != seg[tra] % 3).all()
    assert set(host["aux"][seg // 3 == 2].tolist()) == {0, 1}
    # line starts - and the starts of the bases - fall on every residue mod 4: the unaligned head and tail of the word copy both run
    start = np.r_[0, np.cumsum([len(x) for x in lines])]
    assert set((start[:-1] % 4).tolist()) == {0, 1, 2, 3}
    base_at = [int(start[k]) + len(lines[k]) - 1 - int(host["aux"][k]) for k in np.flatnonzero(ins).tolist()]
    assert {x % 4 for x in base_at} == {0, 1, 2, 3}
    r0, r1 = rebuild.type_row_ranges(cnt, 3)["INS"]
    mid = (r0 + 7, r1 + 11)                                                            # starts and ends mid-type
    for lo, hi in ((0, 1), (0, 1023), (0, 1024), (0, 1025), (0, 2049), (0, n), (1500, 1500), (n, n), mid, (n - 1, n)):
        got = rebuild.sigs_text(ctx, CRAFTED_CHROMS, lo, hi)
        assert got == b"".join(lines[lo:hi]), (lo, hi)
    assert rebuild.sigs_text_host(host, rows["names"], first, rows["seqs"], CRAFTED_CHROMS, *mid) == b"".join(lines[mid[0]:mid[1]])
    chunks = [rebuild.sigs_text(ctx, CRAFTED_CHROMS, lo, min(n, lo + 256)) for lo in range(0, n, 256)]
    assert b"".join(chunks) == b"".join(lines)
    # other strand strings, and a raw result
    timing = {}
    raw = rebuild.sigs_text(ctx, CRAFTED_CHROMS, 0, n, strands=("+", "minus"), raw=True, timing=timing)
    assert raw.tobytes() == rebuild.sigs_text_host(host, rows["names"], first, rows["seqs"], CRAFTED_CHROMS, 0, n, strands=("+", "minus"))
    assert timing["ms_kernels"] > 0


@pytest.mark.gpu
def test_gpu_write_sigs_writes_the_references_files(ctx, tmp_path):
    for name, per, _, sigs in golden_cases():
        chroms = case_chroms(per)
        variants = [("", per, sigs)]
        if name == "crafted":                                  # a type without rows: an empty file, the others unchanged
            variants.append(("_no_dup", dict(per, DUP=[]), dict(sigs, DUP="")))
        for tag, cand, want in variants:
            sigs_helpers.fill_pools(ctx, sigs_helpers.case_rows(cand, chroms))
            rb = sigs_helpers.kept_rebuild(ctx, len(chroms))
            d = tmp_path / (name + tag)
            d.mkdir()
            written = rebuild.write_sigs(ctx, rb, chroms, str(d), rows_per_chunk=100)
            assert sorted(os.listdir(d)) == sorted(t + ".sigs" for t in TYPES)
            for t in TYPES:
                with open(d / (t + ".sigs"), "rb") as f:
                    got = f.read()
                assert got == want[t].encode(), (name, tag, t)
                assert written[t] == len(got)


def _raw_call(ctx, chroms, lo, hi, buf, cap):
    blob, off = rebuild._chrom_table(chroms)
    need = C.c_int64(-1)
    rc = _lib.lib().csv_pool_sigs_text(ctx._h, lo, hi, blob, off.ctypes.data, len(chroms), b"++", b"--", buf.ctypes.data, cap, C.byref(need), None)
    return rc, int(need.value)


@pytest.mark.gpu
def test_gpu_capacity_and_refusals(crafted):
    from cutesv_amd import engine
    from cutesv_amd.engine import CsvError
    want = b"".join(crafted[4][:300])
    chroms = ["c0", "c1"]
    with engine.Context(0) as c2:
        def refused(lo=0, hi=1, chroms=chroms, match=None):
            buf = np.full(4096, 0xAA, np.uint8)
            rc, _ = _raw_call(c2, chroms, lo, hi, buf, len(buf))
            assert rc == _abi.E_INVALID and (buf == 0xAA).all(), (lo, hi)
            with pytest.raises(CsvError, match=match) as e:
                rebuild.sigs_text(c2, chroms, lo, hi)
            assert e.value.code == _abi.E_INVALID

        def pool(seg, a, b, aux, seqs=None):
            sigs_helpers.fill_pools(c2, dict(seg=seg, a=a, b=b, aux=aux, names=[b"n%d" % k for k in range(len(a))], seqs=seqs or {}, halves={}))
        refused(match="no kept pool rebuild")                                          # before any rebuild
        # the crafted pool once more in this context: capacity
        sigs_helpers.fill_pools(c2, crafted[0])
        sigs_helpers.kept_rebuild(c2, 3)
        buf = np.full(len(want) + 64, 0xAA, np.uint8)
        rc, need = _raw_call(c2, CRAFTED_CHROMS, 0, 300, buf, len(want) - 1)
        assert rc == _abi.E_CAPACITY and need == len(want) and (buf == 0xAA).all()
        rc, need = _raw_call(c2, CRAFTED_CHROMS, 0, 300, buf, len(want))
        assert rc == _abi.OK and need == len(want) and buf[:need].tobytes() == want and (buf[need:] == 0xAA).all()
        n = rebuild.pool_rows(c2)
        refused(0, n + 1, CRAFTED_CHROMS, match="outside")                              # the range lies past the rows (n >= n_out)
        refused(5, 4, CRAFTED_CHROMS, match="outside")
        refused(-1, 4, CRAFTED_CHROMS, match="outside")
        assert rebuild.sigs_text(c2, CRAFTED_CHROMS, 0, 300) == want
        rebuild.pool_append(c2, [0], [7], [7], [0], [0])                                # the pool was appended to after the rebuild
        refused(0, 1, CRAFTED_CHROMS, match="changed after the kept rebuild")
        rb2 = sigs_helpers.kept_rebuild(c2, 3)                                          # a new rebuild, which holds the appended row
        got = rebuild.sigs_text(c2, CRAFTED_CHROMS, 0, rb2["n_out"])
        assert got.count(b"\n") == len(crafted[4]) + 1 and b"\nDEL\t1\t7\t7\t" + crafted[0]["names"][0] + b"\n" in got
        # the status bits: two contigs, so DEL = segments 0 1, INS 2 3, INV 4 5, DUP 6 7, TRA 8 9
        pool([0, 1], [5, -1], [6, 6], [0, 0])                                          # a negative a: the rebuild itself refuses the pool,
        with pytest.raises(CsvError):                                                   # so nothing is kept and the entry refuses too
            sigs_helpers.kept_rebuild(c2, 2)
        refused(0, 1)
        pool([0, 1], [5, 1 << 42], [6, 6], [0, 0])
        sigs_helpers.kept_rebuild(c2, 2)
        refused(0, 2, match="2\\^42")
        assert rebuild.sigs_text(c2, chroms, 0, 1) == b"DEL\tc0\t5\t6\tn0\n"             # (the row in front of it is in order)
        pool([0, 2, 3], [5, 5, 5], [6, 6, 6], [0, 4, 4], {1: "ACGT"})                   # an INS row without a sequence
        sigs_helpers.kept_rebuild(c2, 2)
        refused(0, 3, match="no sequence")
        assert rebuild.sigs_text(c2, chroms, 0, 2) == b"DEL\tc0\t5\t6\tn0\nINS\tc0\t5\t6\tn1\tACGT\n"
        pool([0, 3], [5, 5], [6, 6], [0, 4])                                            # ... and no sequence pool at all
        sigs_helpers.kept_rebuild(c2, 2)
        refused(0, 2, match="no sequence")
        for aux, what in ((5, "TRA"), (2 * 8 + 1, "TRA")):                              # a TRA aux with type 5, with chr2 = n_chrom
            pool([8, 9], [5, 5], [6, 6], [0 * 8 + 3, aux])
            sigs_helpers.kept_rebuild(c2, 2)
            refused(0, 2, match=what)
            assert rebuild.sigs_text(c2, chroms, 0, 1) == b"TRA\tc0\tD\t5\tc0\t6\tn0\n"
        pool([4, 4], [5, 5], [6, 6], [1, 2])                                            # an INV strand code above 1
        sigs_helpers.kept_rebuild(c2, 2)
        refused(0, 2, match="strand")
        pool([0, 9], [5, 5], [6, 6], [0, 0])                                            # a segment outside 5 * n_chrom: one contig named, two numbered
        sigs_helpers.kept_rebuild(c2, 2)
        refused(0, 2, chroms=["c0"], match="segment")
        # a rebuild that is not by name, and one that keeps nothing
        _, _, major, nodedup = rebuild._segments(chroms, True)
        rebuild.rebuild_pool(c2, np.arange(2, dtype=np.int32), major, nodedup, keep_on_device=True, ties="seqs")
        refused(0, 1, match="ranks of the name pool")
        rebuild.rebuild_pool_by_name(c2, major, nodedup, keep_on_device=False, ties="seqs")
        refused(0, 1)
        # ... and the context goes on
        sigs_helpers.fill_pools(c2, crafted[0])
        sigs_helpers.kept_rebuild(c2, 3)
        assert rebuild.sigs_text(c2, CRAFTED_CHROMS, 0, 300) == want


# ------------------------------------------------------------------------------------------------ GPU: call_bam(sigs_dir=...)
@pytest.mark.gpu
def test_gpu_call_bam_writes_the_sigs_files_and_the_same_text(ctx, tmp_path):
    path = str(tmp_path / "planted.bam")
    ref = call_helpers.write_planted_bam(path)
    cp = call.CallParams(Params.ont(min_support=3))
    d = tmp_path / "sigs"
    d.mkdir()
    timings = {}
    with bam.BamFile(path) as bf:
        plain, sv0 = call.call_bam(bf, ref, cp, ctx=ctx, report_readid=True)
        text, sv1 = call.call_bam(bf, ref, cp, ctx=ctx, report_readid=True, sigs_dir=str(d), timings=timings)
        assert text == plain and sv0.tolist() == sv1.tolist() and text.count("\n") >= 5
        assert timings["ms_sigs"] > 0
        # the pools of that call are still the context's: the same rebuild, downloaded, through the twin
        chroms = sorted(bf.references)
        host, first = sigs_helpers.host_rebuild(ctx, len(chroms))
        names = rebuild.name_pool_get(ctx, np.arange(rebuild.name_pool_rows(ctx)), raw=True)
        ins_rows = np.flatnonzero(host["seg_id"] // len(chroms) == TYPES.index("INS"))
        seqs = dict(zip(host["src_row"][ins_rows].tolist(), rebuild.seq_pool_get(ctx, host["src_row"][ins_rows])))
        ranges = rebuild.type_row_ranges(np.bincount(host["seg_id"], minlength=5 * len(chroms)), len(chroms))
        got = {}
        for t in TYPES:
            with open(d / (t + ".sigs"), "rb") as f:
                got[t] = f.read()
            assert got[t] == rebuild.sigs_text_host(host, names, first, seqs, chroms, *ranges[t]), t
        assert sorted(os.listdir(d)) == sorted(t + ".sigs" for t in TYPES)
        assert all(got[t] for t in ("DEL", "INS", "DUP", "TRA"))
        # the INS lines carry the bases the host route reports for the same rows
        crank = {c: i for i, c in enumerate(chroms)}
        length = dict(zip(bf.references, bf.lengths))
        cand = [x for c in chroms for x in extract.single_pipe_bam(ctx, bf, c, 0, length[c], crank, *cp.pipe_args())[0]["INS"]]
    by_key = {}
    for x in cand:
        by_key.setdefault((x[-1], int(x[0]), int(x[1]), x[2]), set()).add(x[3])
    ins_lines = [ln.split("\t") for ln in got["INS"].decode().splitlines()]
    assert len(ins_lines) >= 18 and any(len(f[5]) == 300 for f in ins_lines)
    for f in ins_lines:
        assert f[5] in by_key[(f[1], int(f[2]), int(f[3]), f[4])], f[:5]
    assert {f[4] for f in ins_lines} >= {"split_rev", "tieA", "tieB"}
