"""BAM -> VCF body in one call (cutesv_amd/call.py): the two device gathers that make the ALT and RNAMES
strings (csv_seq_alt_gather, csv_name_support_join; cutesv_amd/csrc/vcf_strings.hip.h) and the entry that connects the chain.

CPU: the interface, the numpy twins against Python slices and joins, emit_records with ready-made blobs against the golden text,
the store-free segment record, the task cut.  GPU: the kernels against the twins (edges, misuse), and call_bam against the route
the same file took before - single_pipe_bam, store_from_unsorted, cluster_batch, emit_records - byte for byte."""
import os
import re

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, call, rebuild, synth, vcf
from cutesv_amd.columns import Params, TYPES, segment_record
from helpers import load_json, store_from_json
from seq_pool_helpers import rebuild_case_pool
import call_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


class _NoContext:
    """a context no library call accepts (every entry returns CSV_E_INVALID for a NULL handle before it looks at anything else):
    rebuild_case_pool then only builds its flat list"""
    _h = None

    def _check(self, rc):
        pass


# ------------------------------------------------------------------------------------------------ CPU: the interface
def test_header_declares_and_lib_binds_the_two_entries():
    with open(os.path.join(ROOT, "include", "cutesv_hip.h")) as f:
        header = f.read()
    names = {n for n, _, _ in _lib.SYMBOLS}
    for entry in ("csv_seq_alt_gather", "csv_name_support_join"):
        assert re.search(r"^int %s\(csv_ctx\* ctx" % entry, header, re.M), entry
        assert entry in names
    L = _lib.lib()
    assert L.csv_abi_version() == _abi.ABI_VERSION == 9
    one = np.zeros(1, np.int64)
    assert L.csv_seq_alt_gather(None, 0, None, None, 0, None, 0, one.ctypes.data) == _abi.E_INVALID
    assert L.csv_name_support_join(None, 0, one.ctypes.data, None, None, None, 0, one.ctypes.data) == _abi.E_INVALID


# ------------------------------------------------------------------------------------------------ CPU: the numpy twins
def test_host_twins_are_python_slices_and_joins():
    rng = np.random.default_rng(3)
    n_ins = 0
    for case in load_json("rebuild_order.json.gz"):
        flat = rebuild_case_pool(_NoContext(), case)[0]
        seqs = {k: x[3] for k, (t, x) in enumerate(flat) if t == "INS"}
        src_row = rng.permutation(len(flat))
        rows = np.flatnonzero(np.isin(src_row, list(seqs)))
        n_ins += len(rows)
        for which in range(5):
            want, clip = [], []
            for r in rows.tolist():
                s = seqs[int(src_row[r])]
                svlen = max(0, (0, 1, len(s) - 1, len(s), len(s) + 7)[which])
                clip.append(svlen); want.append(s[:svlen])
            blob, off = rebuild.alt_gather_host(seqs, src_row, rows, clip)
            assert blob == "".join(want).encode() and off.tolist() == np.r_[0, np.cumsum([len(w) for w in want])].tolist(), (case["name"], which)
        with pytest.raises(ValueError):
            rebuild.alt_gather_host(seqs, src_row, rows[:1], [-1])
        with pytest.raises(ValueError):
            rebuild.alt_gather_host(seqs, src_row, [len(src_row)], [3])
        with pytest.raises(ValueError):
            rebuild.alt_gather_host(seqs, src_row, rows[:2], [3])
        other = np.flatnonzero(~np.isin(src_row, list(seqs)))
        if len(other):
            with pytest.raises(ValueError):
                rebuild.alt_gather_host(seqs, src_row, other[:1], [3])
        # the join: names by pool read index, ranks and first as name_ranks_host makes them
        npos = {"DEL": 2, "INS": 2, "DUP": 2, "INV": 3, "TRA": 4}
        names = [x[npos[t]] for t, x in flat]
        data = "".join(names).encode()
        ln = np.asarray([len(x) for x in names]); at = np.cumsum(ln) - ln
        rank, first = rebuild.name_ranks_host(data, at, ln)
        read_id = rank[src_row]
        sizes = rng.integers(0, 6, 40)
        soff = np.r_[0, np.cumsum(sizes)]
        sup = rng.integers(0, len(flat), int(soff[-1]))
        blob, off = rebuild.support_join_host(names, first, read_id, soff, sup)
        want = [",".join(names[int(src_row[s])] for s in sup[soff[c]:soff[c + 1]]) for c in range(40)]
        assert blob == "".join(want).encode() and off.tolist() == np.r_[0, np.cumsum([len(w) for w in want])].tolist(), case["name"]
        assert (sizes == 0).any() and (sizes > 1).any()
        with pytest.raises(ValueError):
            rebuild.support_join_host(names, first, read_id, [1, 2], sup)
        with pytest.raises(ValueError):
            rebuild.support_join_host(names, first, read_id, [0, 2, 1], sup)
        with pytest.raises(ValueError):
            rebuild.support_join_host(names, first, read_id, [0, len(sup) + 1], sup)
        with pytest.raises(ValueError):
            rebuild.support_join_host(names, first, read_id, [0, 1], [len(flat)])
    assert n_ins > 100


# ------------------------------------------------------------------------------------------------ CPU: emit_records with blobs
def _host_blobs(st, segs, res):
    """ins_alt / rnames of a result, from the store's own tables"""
    t = res.trimmed()
    ins = np.flatnonzero(segs["svtype"][t["call_seg"]] == _abi.INS)
    alts = [st.sequence(int(pk))[:int(ln)].encode() for pk, ln in zip(t["seq_pick"][ins], t["bp2"][ins])]
    nm = st.names.take(st.read_id[t["support_sig"]])
    so = t["support_off"].tolist()
    rn = [",".join(nm[so[c]:so[c + 1]]).encode() for c in range(res.n_calls)]
    return (b"".join(alts), np.asarray([len(a) for a in alts], np.int64)), (b"".join(rn), np.r_[0, np.cumsum([len(x) for x in rn])].astype(np.int64))


def test_emit_records_takes_ready_made_alt_and_rnames_blobs():
    from oracle import oracle
    from test_vcf_emit import _canon
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    n_alt = n_rn = 0
    for g in load_json("vcf_lines.json.gz"):
        case = small[g["case"]]
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        hb = st.host_batch([(t, c) for t, c, _ in case["rows"]], p)
        res = oracle.cluster_batch(hb, per_sig=False)
        kw = dict(min_size=p.min_size, max_size=p.max_size, genotype=p.genotype, **g["flags"])
        plain, sv0 = vcf.emit_records(st, hb.segments, res, ref, **kw)
        ins_alt, rnames = _host_blobs(st, hb.segments, res)
        shim = call._Shim(st.chroms, st.strands)                  # (nothing but chroms and strands is read of the store)
        text, sv1 = vcf.emit_records(shim, hb.segments, res, ref, ins_alt=ins_alt, rnames=rnames, **kw)
        assert text == plain and sv0.tolist() == sv1.tolist(), (g["case"], g["flags"])
        assert _canon(text) == _canon(g["text"]), (g["case"], g["flags"])       # (the golden text, up to the order of the reference's name sets)
        n_alt += len(ins_alt[0]); n_rn += len(rnames[0]) if g["flags"].get("report_readid") else 0
        if len(ins_alt[1]) and not g["flags"].get("ignore_sequence"):
            with pytest.raises(ValueError):
                vcf.emit_records(shim, hb.segments, res, ref, ins_alt=(ins_alt[0], ins_alt[1][:-1]), rnames=rnames, **kw)
            with pytest.raises(ValueError):
                vcf.emit_records(shim, hb.segments, res, ref, ins_alt=(ins_alt[0] + b"A", ins_alt[1]), rnames=rnames, **kw)
        if g["flags"].get("report_readid") and res.n_calls:
            with pytest.raises(ValueError):
                vcf.emit_records(shim, hb.segments, res, ref, ins_alt=ins_alt, rnames=(rnames[0], rnames[1][:-1]), **kw)
            with pytest.raises(ValueError):
                vcf.emit_records(shim, hb.segments, res, ref, ins_alt=ins_alt, rnames=(rnames[0] + b"x", rnames[1]), **kw)
    assert n_alt > 0 and n_rn > 0


# ------------------------------------------------------------------------------------------------ CPU: segment records, task cut
def test_segment_record_is_sigstore_segment():
    seen = set()
    for case in load_json("small_cases.json.gz"):
        st = store_from_json(case["store"])
        base = Params(**case["params"])
        for p in (base, Params.ont(min_support=3, genotype=True), Params.hifi(min_support=2, genotype=True, genotype_tra=st.contig_len is not None)):
            for (t, ch), (beg, end) in st.seg_index.items():
                want = st.segment(t, ch, p)
                got = segment_record(t, st.chroms.index(ch), beg, end, p, have_contig_len=st.contig_len is not None)
                for name in _abi.SEGMENT_DTYPE.names:
                    assert got[name] == want[name], (case["name"], t, ch, name)
                seen.add(t)
    assert seen == set(TYPES)
    with pytest.raises(ValueError):
        segment_record("TRA", 0, 0, 1, Params(genotype=True, genotype_tra=True), have_contig_len=False)


def reference_tasks(length, batch):
    """the task cut of the reference's main_ctrl with a fixed batch, restated"""
    if length < batch:
        return [(0, length)]
    out, pos = [], 0
    for _ in range(int(length / batch)):
        out.append((pos, pos + batch)); pos += batch
    if pos < length:
        out.append((pos, length))
    return out


def test_task_cut_is_the_references():
    B = 1000
    for L in (1, B - 1, B, B + 1, 3 * B):
        assert call.cut_tasks(L, B) == reference_tasks(L, B), L
    assert call.cut_tasks(3 * B, B) == [(0, B), (B, 2 * B), (2 * B, 3 * B)] and call.cut_tasks(B + 1, B) == [(0, B), (B, B + 1)]
    with pytest.raises(ValueError):
        call.cut_tasks(10, 0)


def test_tra_genotyping_modes(monkeypatch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "bam")
    assert call.tra_gt_mode(False) == "off"
    with pytest.raises(ValueError) as e:
        call.tra_gt_mode(True)
    assert "reads_table" in str(e.value) and "off" in str(e.value)
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "reads_table")
    assert call.tra_gt_mode(True) == "reads_table"


# ------------------------------------------------------------------------------------------------ GPU: the alt gather
def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


ALT_LENS = (0, 1, 3, 4, 5, 255, 256, 257, 1031)


def alt_pool(ctx):
    """INS rows of ALT_LENS bases (pool rows 0 ..) and a DEL row behind them, names for their reads, rebuilt by name and kept
    -> (sequences by pool row, the rebuild)"""
    rng = np.random.default_rng(17)
    seqs = {k: _bases(rng, n) for k, n in enumerate(ALT_LENS)}
    n = len(ALT_LENS)
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    rebuild.pool_append(ctx, [0] * n + [1], 1000 * np.arange(n + 1)[::-1], [len(seqs[k]) for k in range(n)] + [50], np.arange(n + 1), [len(seqs[k]) for k in range(n)] + [0])
    rebuild.seq_pool_put(ctx, np.arange(n), [seqs[k] for k in range(n)])
    names = ["q%02d" % k for k in range(n + 1)]
    rebuild.name_pool_append(ctx, "".join(names).encode(), 3 * np.arange(n + 1), np.full(n + 1, 3))
    rb = rebuild.rebuild_pool_by_name(ctx, np.zeros(2, np.uint8), np.asarray([1, 0], np.uint8), keep_on_device=True, ties="seqs")
    assert rb["n_out"] == n + 1
    return seqs, rb


@pytest.mark.gpu
def test_gpu_alt_gather_edges(ctx):
    seqs, rb = alt_pool(ctx)
    src = rb["src_row"]
    ins_rows = np.flatnonzero(src < len(ALT_LENS))
    assert src[ins_rows].tolist() != sorted(src[ins_rows].tolist())                       # (the rebuild moved the rows: src_row is not the identity)
    none = rebuild.alt_gather(ctx, [], [])
    assert none[0] == b"" and none[1].tolist() == [0]
    pick, clip = [], []
    for r in ins_rows.tolist():
        ln = len(seqs[int(src[r])])
        for c in sorted({0, 1, max(0, ln - 1), ln, ln + 1}):
            pick.append(r); clip.append(c)
    pick, clip = np.asarray(pick + pick[::-1] + pick[:7] * 3), np.asarray(clip + clip[::-1] + clip[:7] * 3)       # in order, reversed, repeated
    want = rebuild.alt_gather_host(seqs, src, pick, clip)
    got = rebuild.alt_gather(ctx, pick, clip)
    assert got[0] == want[0] and got[1].tolist() == want[1].tolist()
    assert len({int(o) & 3 for o in want[1]}) == 4 and int(np.diff(want[1]).max()) == 1031      # every alignment of the first byte; more than one round of 64 x 4
    got32 = rebuild.alt_gather(ctx, pick.astype(np.int32), clip.astype(np.int32), raw=True)
    assert got32[0].tobytes() == want[0] and got32[1].tolist() == want[1].tolist()
    one = rebuild.alt_gather(ctx, pick[5:6], clip[5:6])
    assert one[0] == want[0][want[1][5]:want[1][6]] and one[1].tolist() == [0, int(want[1][6] - want[1][5])]
    # 70 000 picks of the short rows: more wavefronts than the capped grid starts
    short = [(p, c) for p, c in zip(pick.tolist(), clip.tolist()) if len(seqs[int(src[p])]) <= 5]
    many = np.asarray(short * (70000 // len(short) + 1))[:70000]
    want = rebuild.alt_gather_host(seqs, src, many[:, 0], many[:, 1])
    got = rebuild.alt_gather(ctx, many[:, 0], many[:, 1])
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: the support join
def join_pool(ctx):
    """one DEL row per name index; names of 1, 63, 64, 65, 254 and 255 bytes, one text at two indices, the rest short
    -> (names, first, read_id of the rebuilt rows, the rebuild)"""
    names = ["a", "b" * 63, "c" * 64, "d" * 65, "e" * 254, "f" * 255, "same_text", "same_text"] + ["n%04d" % k for k in range(302)]
    n = len(names)
    ln = np.asarray([len(x) for x in names])
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)
    rebuild.pool_append(ctx, [0] * n, 100 * np.arange(n)[::-1], [40] * n, np.arange(n), [0] * n)
    rebuild.name_pool_append(ctx, "".join(names).encode(), np.cumsum(ln) - ln, ln)
    rb = rebuild.rebuild_pool_by_name(ctx, np.zeros(1, np.uint8), np.zeros(1, np.uint8), keep_on_device=True)
    ranks = rebuild.name_ranks(ctx)
    assert rb["n_out"] == n and ranks["n_distinct"] == n - 1
    return names, ranks["first"], ranks["rank"][rb["src_row"]], rb


@pytest.mark.gpu
def test_gpu_support_join_edges(ctx):
    names, first, read_id, rb = join_pool(ctx)
    n = len(names)
    row_of = np.argsort(rb["src_row"])                              # rebuilt row of pool row k (= name index k)
    calls = [[row_of[4]], [row_of[5], row_of[0]], [], list(row_of[:65]), list(row_of[8:308]), [], [row_of[3], row_of[3]], [row_of[6], row_of[7]], [row_of[1], row_of[2]]]
    soff = np.r_[0, np.cumsum([len(c) for c in calls])]
    sup = np.asarray([s for c in calls for s in c], np.int64)
    want = rebuild.support_join_host(names, first, read_id, soff, sup)
    text = want[0].decode()
    assert text[want[1][6]:want[1][7]] == "d" * 65 + "," + "d" * 65 and text[want[1][7]:want[1][8]] == "same_text,same_text"
    assert want[1][2] == want[1][3] and want[1][5] == want[1][6] and text.startswith("e" * 254 + "f" * 255 + ",a")
    got = rebuild.support_join(ctx, soff, sup)
    assert got[0] == want[0] and got[1].tolist() == want[1].tolist()
    got32 = rebuild.support_join(ctx, soff, sup.astype(np.int32), raw=True)
    assert got32[0].tobytes() == want[0] and got32[1].tolist() == want[1].tolist()
    empty = rebuild.support_join(ctx, [0, 0, 0], [])
    assert empty[0] == b"" and empty[1].tolist() == [0, 0, 0]
    # 70 000 supports in one batch, calls of 0 .. 13 supports
    rng = np.random.default_rng(4)
    sizes = rng.integers(0, 14, 12000)
    soff = np.r_[0, np.cumsum(sizes)]
    soff = soff[:int(np.searchsorted(soff, 70000))]
    soff = np.r_[soff, 70000]
    sup = rng.integers(0, n, 70000)
    want = rebuild.support_join_host(names, first, read_id, soff, sup)
    got = rebuild.support_join(ctx, soff, sup)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU: misuse
@pytest.mark.gpu
def test_gpu_misuse_leaves_the_context_and_the_pools_usable():
    from cutesv_amd import engine
    from cutesv_amd.engine import CsvError
    L = _lib.lib()
    with engine.Context(0) as c2:
        def counts():
            return rebuild.pool_rows(c2), rebuild.seq_pool_rows(c2), rebuild.name_pool_rows(c2)

        def refused(fn, *a):
            before = counts()
            with pytest.raises(CsvError) as e:
                fn(c2, *a)
            assert e.value.code == _abi.E_INVALID, e.value
            assert counts() == before
        # before any rebuild
        refused(rebuild.alt_gather, [0], [1])
        refused(rebuild.support_join, [0, 1], [0])
        seqs, rb = alt_pool(c2)
        src = rb["src_row"]
        ins_rows, del_row = np.flatnonzero(src < len(ALT_LENS)), int(np.flatnonzero(src == len(ALT_LENS))[0])
        clip = np.full(len(ins_rows), 300)
        want = rebuild.alt_gather_host(seqs, src, ins_rows, clip)
        soff, sup = [0, 2, 3], [del_row, int(ins_rows[0]), int(ins_rows[1])]
        want_rn = rebuild.support_join_host(["q%02d" % k for k in range(len(ALT_LENS) + 1)], np.arange(len(ALT_LENS) + 1), src, soff, sup)      # (names are distinct and sorted: rank = index)

        def works():
            got = rebuild.alt_gather(c2, ins_rows, clip)
            assert got[0] == want[0] and got[1].tolist() == want[1].tolist()
            got = rebuild.support_join(c2, soff, sup)
            assert got[0] == want_rn[0] and got[1].tolist() == want_rn[1].tolist()
        works()
        # argument errors: nothing is launched for the first two, the third is found by the length pass
        for bad in (([int(ins_rows[0])], [-1]), ([rb["n_out"]], [5]), ([-1], [5]), ([del_row], [5])):
            refused(rebuild.alt_gather, *bad)
            works()
        for bad in (([0, 1], [rb["n_out"]]), ([0, 1], [-1]), ([1, 2], sup), ([0, 2, 1], sup)):
            refused(rebuild.support_join, *bad)
            works()
        # a capacity that is too small reports the need, and the call then succeeds
        off = np.zeros(len(ins_rows) + 1, np.int64)
        out = np.zeros(len(want[0]), np.uint8)
        p64, c64 = ins_rows.astype(np.int64), clip.astype(np.int64)
        assert L.csv_seq_alt_gather(c2._h, len(p64), p64.ctypes.data, c64.ctypes.data, 0, out.ctypes.data, 1, off.ctypes.data) == _abi.E_CAPACITY
        assert off[-1] == len(want[0]) and not out.any()
        assert L.csv_seq_alt_gather(c2._h, len(p64), p64.ctypes.data, c64.ctypes.data, 0, out.ctypes.data, len(out), off.ctypes.data) == _abi.OK
        assert out.tobytes() == want[0]
        so, sp = np.asarray(soff, np.int64), np.asarray(sup, np.int64)
        off, out = np.zeros(3, np.int64), np.zeros(len(want_rn[0]), np.uint8)
        assert L.csv_name_support_join(c2._h, 2, so.ctypes.data, sp.ctypes.data, None, out.ctypes.data, 2, off.ctypes.data) == _abi.E_CAPACITY
        assert off[-1] == len(want_rn[0]) and not out.any()
        assert L.csv_name_support_join(c2._h, 2, so.ctypes.data, sp.ctypes.data, None, out.ctypes.data, len(out), off.ctypes.data) == _abi.OK
        assert out.tobytes() == want_rn[0]
        works()
        # a rebuild without the name pool's ranks: the ALT works, the join does not
        ident = np.arange(len(ALT_LENS) + 1, dtype=np.int32)
        rb2 = rebuild.rebuild_pool(c2, ident, np.zeros(2, np.uint8), np.asarray([1, 0], np.uint8), keep_on_device=True, ties="seqs")
        assert np.array_equal(rb2["src_row"], src)
        refused(rebuild.support_join, soff, sup)
        got = rebuild.alt_gather(c2, ins_rows, clip)
        assert got[0] == want[0]
        # a rebuild that keeps nothing on the device leaves nothing to gather from
        rebuild.rebuild_pool_by_name(c2, np.zeros(2, np.uint8), np.asarray([1, 0], np.uint8), keep_on_device=False, ties="seqs")
        refused(rebuild.alt_gather, ins_rows, clip)
        # a pool append / a name append after the kept rebuild
        for change in (lambda: rebuild.pool_append(c2, [1], [7], [7], [0], [0]), lambda: rebuild.name_pool_append(c2, b"zz", [0], [2]), lambda: rebuild.pool_reset(c2)):
            rebuild.rebuild_pool_by_name(c2, np.zeros(2, np.uint8), np.asarray([1, 0], np.uint8), keep_on_device=True, ties="seqs")
            assert rebuild.alt_gather(c2, ins_rows[:1], [3])[1].tolist()[0] == 0
            change()
            refused(rebuild.alt_gather, ins_rows[:1], [3])
            refused(rebuild.support_join, [0, 1], [0])
        # ... and the context goes on: a new pool, a new rebuild, the right bytes
        alt_pool(c2)
        works()


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("call") / "planted.bam")
    return path, call_helpers.write_planted_bam(path)


def _records(text):
    return [ln.split("\t") for ln in text.splitlines()]


@pytest.mark.gpu
@pytest.mark.parametrize("genotype,report_readid,batch", [(False, False, 10_000_000), (True, False, 10_000_000), (True, True, 10_000_000), (False, False, 2000),
                                                           (True, True, 2000)])
def test_gpu_call_bam_is_the_route_through_the_store(ctx, planted, monkeypatch, genotype, report_readid, batch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "reads_table")
    path, ref = planted
    cp = call.CallParams(Params.ont(min_support=3, genotype=genotype))
    with bam.BamFile(path) as bf:
        want = call_helpers.parent_route(ctx, bf, ref, cp, batch=batch, report_readid=report_readid)
        got, svid = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid)
        again, _ = call.call_bam(bf, ref, cp, ctx=ctx, batch=batch, report_readid=report_readid)       # (the pools were reset)
    # the expected text holds what was planted: equality cannot be vacuous
    recs = _records(want)
    kinds = [re.search(r"SVTYPE=(\w+)", r[7]).group(1) for r in recs]
    assert sum(1 for r, k in zip(recs, kinds) if k == "INS" and len(r[4]) > 100) >= 2
    assert kinds.count("DEL") >= 1 and kinds.count("DUP") >= 1 and kinds.count("BND") >= 1
    if report_readid:
        assert all(re.search(r"RNAMES=[^;\t]+", r[7]) for r in recs)
    else:
        assert all("RNAMES=" not in r[7] or "RNAMES=NULL" in r[7] for r in recs)
    if genotype:
        assert any(r[9].split(":")[0] != "./." for r in recs)
    assert got == want
    assert again == got
    assert int(svid.sum()) == len(recs)
    if report_readid:
        assert "split_rev" in want and "tieA" in want


@pytest.mark.gpu
def test_gpu_call_bam_from_a_path_and_the_command_line(planted, tmp_path, monkeypatch):
    """a path instead of an open file, a context of its own, ignore_sequence, one contig only; and the module's main()"""
    path, ref = planted
    cp = call.CallParams(Params.ont(min_support=3))
    text, svid = call.call_bam(path, ref, cp)
    plain, _ = call.call_bam(path, ref, cp, ignore_sequence=True)
    assert "<INS>" in plain and "<INS>" not in text and text.count("\n") == plain.count("\n") == int(svid.sum())
    only_b, _ = call.call_bam(path, ref, cp, chroms=["chrB"])
    assert only_b == ""
    with pytest.raises(KeyError):
        call.call_bam(path, ref, cp, chroms=["chrZ"])
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "bam")
    with pytest.raises(ValueError):
        call.call_bam(path, ref, call.CallParams(Params.ont(min_support=3, genotype=True)))
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n" % c + "\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    out = str(tmp_path / "out.body.vcf")
    assert call.main([path, fa, "-o", out, "--preset", "ont", "--min_support", "3"]) == 0
    with open(out) as f:
        assert f.read() == text


@pytest.mark.gpu
def test_gpu_call_bam_fills_timings_in_the_order_of_its_phases(ctx, planted, tmp_path):
    """the keys of `timings` in insertion order, which is the order the command line logs them in: the sums over the tasks, then one lap per
    phase; ms_sigs only with sigs_dir, ms_index in front with index="build", nothing after ms_tasks when the pool stays empty, and the same
    keys however many tasks a contig is cut into"""
    path, ref = planted
    cp = call.CallParams(Params.ont(min_support=3))
    tasks = ["ms_inflate", "ms_frame", "ms_tasks"]
    tail = ["ms_cluster", "ms_tra_gt", "ms_alt_gather", "ms_support_join", "ms_emit"]
    seen = {}
    with bam.BamFile(path) as bf:
        for name, kw in (("defaults", {}), ("sigs", dict(sigs_dir=str(tmp_path))), ("empty", dict(chroms=["chrB"])), ("many tasks", dict(batch=2000))):
            seen[name] = {}
            text, _ = call.call_bam(bf, ref, cp, ctx=ctx, timings=seen[name], **kw)
            assert (text == "") == (name == "empty")
    seen["build"] = {}
    call.call_bam(path, ref, cp, ctx=ctx, index="build", timings=seen["build"])
    assert list(seen["defaults"]) == tasks + ["ms_rebuild"] + tail
    assert list(seen["sigs"]) == tasks + ["ms_rebuild", "ms_sigs"] + tail
    assert list(seen["build"]) == ["ms_index"] + tasks + ["ms_rebuild"] + tail
    assert list(seen["empty"]) == tasks
    assert list(seen["many tasks"]) == list(seen["defaults"])
    assert all(isinstance(v, float) and v >= 0 for t in seen.values() for v in t.values())
