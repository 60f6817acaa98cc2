"""resolve.phase3: the reference's phase 3 (main script :1113-1199) on its own work directory in one call - the pickles walked in
C on host threads without the interpreter lock (SigStore.from_reference_workdir_native), one csv_cluster_batch per device.

CPU part: the store against from_reference_workdir, the rows against the reference's digests and the reference model's pool
(oracle/py_restatement under main_ctrl_phase3), with the C oracle standing in for the device.
GPU part (`-m gpu`): the same in a fresh interpreter on the MI355X (tests/phase3_main.py)."""
import json
import os
import pickle
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from cutesv_amd import resolve, synth, vcf, _cols_native as cn
from cutesv_amd.columns import Params, SigStore, TYPES, _WALK
from cutesv_amd.phase3 import digests, main as cli_main
from helpers import load_json, store_from_json, assert_rows_equal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RUNNER = os.path.join(HERE, "phase3_main.py")
CFGS = {"cfg3_s025": lambda: synth.ont30(scale=0.25), "cfg4_s002": lambda: synth.hifi30_gt(scale=0.02),
        "cfg5_s002": lambda: synth.ont90_all(scale=0.02)}


class _OracleCtx:
    """stands in for engine.Context where only csv_cluster_batch's result matters"""

    def cluster_batch(self, hb, reuse=False, **kw):
        from oracle import oracle
        return oracle.cluster_batch(hb, per_sig=False)


_wd_cache = {}


def _workdir(tmp_path_factory, cfg):
    if cfg not in _wd_cache:
        st = CFGS[cfg]()
        wd = str(tmp_path_factory.mktemp(cfg)) + "/"
        _wd_cache[cfg] = (st, wd, st.write_reference_workdir(wd))
    return _wd_cache[cfg]


def _assert_same_store(A, B):
    assert A.chroms == B.chroms
    assert list(A.seg_index.items()) == list(B.seg_index.items())
    for k in ("a", "b", "aux"):
        assert np.array_equal(getattr(A, k), getattr(B, k)), k
    assert tuple(A.strands) == tuple(B.strands)
    assert A.names.take(A.read_id) == B.names.take(B.read_id)
    for (t, _), (lo, hi) in A.seg_index.items():
        if t == "INS":
            assert [A.sequence(i) for i in range(lo, hi)] == [B.sequence(i) for i in range(lo, hi)]
    assert (A.reads_off is None) == (B.reads_off is None)
    if A.reads_off is not None:
        for k in ("reads_off", "r_start", "r_end", "r_primary"):
            assert np.array_equal(getattr(A, k), getattr(B, k)), k
        assert A.names.take(A.r_id) == B.names.take(B.r_id)


def _by_type(results):
    per = {}
    for ch, rows in results.items():
        for r in rows:
            t = r[1] if r[1] in ("DEL", "INS", "DUP", "INV") else "TRA"
            per.setdefault("%s:%s" % (t, ch), []).append(r)
    return per


# ------------------------------------------------------------------------------------------------ the store
def test_native_walk_builds_the_store_of_from_reference_workdir(tmp_path, tmp_path_factory):
    # (work directories in the rebuild's order, as the reference writes them: from_reference_workdir sorts, the reference's phase
    # 3 - and the native walk - take the files' order)
    for case in load_json("small_cases.json.gz"):
        wd = str(tmp_path / case["name"]) + "/"
        os.makedirs(wd + "unsorted")
        st = store_from_json(case["store"])
        idx = SigStore.from_reference_workdir(wd + "unsorted/", st.write_reference_workdir(wd + "unsorted/")).write_reference_workdir(wd)
        B = SigStore.from_reference_workdir_native(wd, idx)
        _assert_same_store(SigStore.from_reference_workdir(wd, idx), B)
        assert B.narrow and "a" in B.narrow and "rows8" in B.narrow           # the one-shot call's int32 / 16-bit forms
        if B.n_reads:
            assert "r_idp" in B.narrow
    for cfg in ("cfg4_s002", "cfg5_s002"):
        _, wd0, idx0 = _workdir(tmp_path_factory, cfg)
        wd = str(tmp_path / cfg) + "/"
        os.makedirs(wd)
        idx = SigStore.from_reference_workdir(wd0, idx0).write_reference_workdir(wd)
        _assert_same_store(SigStore.from_reference_workdir(wd, idx), SigStore.from_reference_workdir_native(wd, idx))


def _store_bytes(st):
    out = [list(st.chroms), sorted(st.seg_index.items()), tuple(st.strands)]
    for k in ("a", "b", "read_id", "aux", "reads_off", "r_start", "r_end", "r_primary", "r_id"):
        v = getattr(st, k)
        out.append(None if v is None else np.asarray(v).tobytes())
    nm = st.names.names
    out += [bytes(memoryview(nm.buf)), nm.off.tobytes(), nm.len.tobytes()]
    out += [st.ins_seq.off.tobytes(), st.ins_seq.len.tobytes()]
    for k in sorted(st.narrow):
        v = st.narrow[k]
        out.append([np.asarray(x).tobytes() for x in v] if isinstance(v, tuple) else np.asarray(v).tobytes())
    return out


def test_thread_counts_give_byte_identical_stores(tmp_path_factory):
    _, wd, idx = _workdir(tmp_path_factory, "cfg5_s002")
    ref = _store_bytes(SigStore.from_reference_workdir_native(wd, idx, threads=1))
    for th in (3, 16):
        assert _store_bytes(SigStore.from_reference_workdir_native(wd, idx, threads=th)) == ref


def _rewrite_block(wd, idx, kind, ch, blk, protocol):
    """append `blk` pickled with `protocol` to <kind>.pickle and point the index at it"""
    with open(wd + kind + ".pickle", "ab") as f:
        off = f.tell()
        pickle.dump(blk, f, protocol=protocol)
    idx = {k: dict(v) for k, v in idx.items()}
    idx[kind][ch] = off
    return idx


def _block(wd, idx, kind, ch):
    with open(wd + kind + ".pickle", "rb") as f:
        f.seek(idx[kind][ch])
        return pickle.load(f)


def test_a_block_the_walker_does_not_know_is_read_by_pickle(tmp_path):
    st, p, case = _golden("ont_gt")
    wd = str(tmp_path) + "/"
    idx = st.write_reference_workdir(wd)
    ch = next(iter(idx["DEL"]))
    want = resolve.phase3(wd, idx, p, ctx=_OracleCtx(), lazy=False)
    # protocol 0 (text opcodes) for one chromosome's DEL block and its reads block
    bad = _rewrite_block(wd, idx, "DEL", ch, _block(wd, idx, "DEL", ch), 0)
    bad = _rewrite_block(wd, bad, "reads", ch, _block(wd, bad, "reads", ch), 0)
    mm = open(wd + "DEL.pickle", "rb").read()
    assert cn.pickle_table(mm, bad["DEL"][ch], *_WALK["DEL"][:3]) is None
    _assert_same_store(SigStore.from_reference_workdir_native(wd, idx), SigStore.from_reference_workdir_native(wd, bad))
    got = resolve.phase3(wd, bad, p, ctx=_OracleCtx(), lazy=False)
    assert got == want


@pytest.fixture(autouse=True)
def _no_tra_bam(monkeypatch):
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "off")        # (the reference's TRA rows of these cases were made with action=False)


# ------------------------------------------------------------------------------------------------ the rows
def _golden(name):
    case = next(c for c in load_json("small_cases.json.gz") if c["name"] == name)
    return store_from_json(case["store"]), Params(**case["params"]), case


@pytest.mark.parametrize("name", ["ont_gt", "realnames_gt", "hifi", "dense_dups"])
def test_phase3_equals_the_reference_models_pool(tmp_path, name):
    """row for row, in order, against main_ctrl_phase3 running oracle/py_restatement's five callables under the forked pool"""
    from oracle import py_restatement as pr
    st, p, case = _golden(name)
    wd = str(tmp_path) + "/"
    idx = st.write_reference_workdir(wd)
    want = resolve.main_ctrl_phase3(wd, idx, p, 3, fns=pr.REF_FNS)
    for lazy in (False, True):
        got = resolve.phase3(wd, idx, p, ctx=_OracleCtx(), lazy=lazy)
        assert list(got) == list(want)                       # the same chromosomes, in main_ctrl's order
        for ch, rows in want.items():
            assert len(got[ch]) == len(rows)
            for g, w in zip(got[ch], rows):
                t = w[1] if w[1] in ("DEL", "INS", "DUP", "INV") else "TRA"
                assert_rows_equal(t, [list(g)], [w], where="%s %s" % (name, ch))


@pytest.mark.parametrize("cfg", ["cfg3_s025", "cfg4_s002", "cfg5_s002"])
def test_phase3_rows_equal_the_reference_digests(tmp_path_factory, cfg):
    st, wd, idx = _workdir(tmp_path_factory, cfg)
    d = load_json("digests.json")[cfg]
    p = Params(**d["params"])
    got = digests(resolve.phase3(wd, idx, p, ctx=_OracleCtx(), lazy=False))
    for key, (n, h) in d["segments"].items():
        if n:
            assert got[key] == [n, h], key
    assert sum(1 for v in got.values() if v[0]) == sum(1 for v in d["segments"].values() if v[0])
    # the other genotyping setting: the same rows as the whole-genome stage on the store the files were written from
    import dataclasses
    q = dataclasses.replace(p, genotype=not p.genotype)
    if cfg == "cfg3_s025" and q.genotype:
        return                                             # (no reads table in this workload)
    want = resolve.cluster_stage(st, q, ctx=_OracleCtx())
    got = resolve.phase3(wd, idx, q, ctx=_OracleCtx(), lazy=False)
    assert digests(got) == digests(want)


def test_a_chromosome_without_reads_block_keeps_the_references_behaviour(tmp_path):
    """INDEL:443-444: a genotyping task whose chromosome has no reads block returns no calls"""
    from oracle import py_restatement as pr
    st, p, case = _golden("ont_gt")
    assert p.genotype
    wd = str(tmp_path) + "/"
    idx = st.write_reference_workdir(wd)
    ch = sorted(idx["reads"])[0]
    del idx["reads"][ch]
    want = resolve.main_ctrl_phase3(wd, idx, p, 2, fns=pr.REF_FNS)
    got = resolve.phase3(wd, idx, p, ctx=_OracleCtx(), lazy=False)
    assert digests(got) == digests(want) and list(got) == list(want)
    assert sum(len(v) for v in got.values()) > 0


def test_two_devices_give_the_rows_of_one(tmp_path_factory):
    _, wd, idx = _workdir(tmp_path_factory, "cfg5_s002")
    p = Params(**load_json("digests.json")["cfg5_s002"]["params"])
    made = []

    def factory(dev):
        made.append(dev)
        return _OracleCtx()
    one = resolve.phase3(wd, idx, p, ctx=_OracleCtx(), lazy=False)
    two = resolve.phase3(wd, idx, p, devices=[0, 0], ctx=factory, lazy=False)
    assert made == [0, 0]
    assert list(two) == list(one) and two == one
    shards = resolve._deal_chromosomes(SigStore.from_reference_workdir_native(wd, idx, reads=False), [(t, c) for t in TYPES for c in idx[t]], 2, False)
    assert all(shards) and not ({c for _, c in shards[0]} & {c for _, c in shards[1]})


def test_the_walk_releases_the_interpreter_lock(tmp_path_factory):
    _, wd, idx = _workdir(tmp_path_factory, "cfg3_s025")
    mm = open(wd + "INS.pickle", "rb").read()
    width, fi, fs, chk, key = _WALK["INS"]
    jobs = tuple((mm, int(off), -1, width, fi, fs, chk, ch.encode(), key) for ch, off in idx["INS"].items()) * 8
    ticks, stop = [0], threading.Event()

    def spin():
        while not stop.is_set():
            ticks[0] += 1
    th = threading.Thread(target=spin)
    th.start()
    try:
        time.sleep(0.05)
        t0 = time.perf_counter()
        before = ticks[0]
        out = cn.walk_workdir(jobs, 1)
        during = ticks[0] - before
        took = time.perf_counter() - t0
    finally:
        stop.set()
        th.join()
    assert all(isinstance(t, tuple) for t in out)
    # with the lock held for the whole call the spinning thread could not have run for more than a switch interval
    assert took > 4 * sys.getswitchinterval() and during > 10000, (took, during)


# ------------------------------------------------------------------------------------------------ the command line
def test_the_cli_writes_emit_stage_of_the_stage(tmp_path):
    st, p, case = _golden("ont_gt")
    wd = str(tmp_path / "wd") + "/"
    os.makedirs(wd)
    st.write_reference_workdir(wd)
    n = int(max(st.a.max(), st.b.max(), st.r_end.max())) + 20000
    ref = {c: synth.reference_sequence(n, seed=7 + i) for i, c in enumerate(st.chroms)}
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n%s\n" % (c, s if isinstance(s, str) else s.decode()))
    out = str(tmp_path / "out.vcf")
    p_ont = Params.ont(genotype=True)
    assert cli_main([wd, "--preset", "ont", "--genotype", "--fasta", fa, "-o", out], ctx=_OracleCtx()) == 0
    want, _ = vcf.emit_stage(resolve.cluster_stage(SigStore.from_reference_workdir(wd), p_ont, ctx=_OracleCtx(), lazy=True), ref,
                             min_size=p_ont.min_size, max_size=p_ont.max_size, genotype=True)
    with open(out) as f:
        got = f.read()
    assert got == want and got.count("\n") > 10
    dg = str(tmp_path / "d.json")
    assert cli_main([wd, "--preset", "ont", "--genotype", "--digest", "-o", dg], ctx=_OracleCtx()) == 0
    with open(dg) as f:
        got = json.load(f)
    with open(wd + "sigindex.pickle", "rb") as f:
        idx = pickle.load(f)
    assert got == digests(resolve.phase3(wd, idx, p_ont, ctx=_OracleCtx(), lazy=False))


def _write_fasta(tmp_path, st):
    n = int(max(st.a.max(), st.b.max(), st.r_end.max())) + 20000
    ref = {c: synth.reference_sequence(n, seed=7 + i) for i, c in enumerate(st.chroms)}
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for c, s in ref.items():
            f.write(">%s\n%s\n" % (c, s if isinstance(s, str) else s.decode()))
    return fa


def test_the_cli_writes_one_body_from_two_devices(tmp_path, monkeypatch):
    """several devices: the devices' results are joined into one, so the VCF body is the one-device body"""
    st, p, case = _golden("realnames_gt")
    wd = str(tmp_path / "wd") + "/"
    os.makedirs(wd)
    idx = st.write_reference_workdir(wd)
    fa = _write_fasta(tmp_path, st)
    one, two = str(tmp_path / "one.vcf"), str(tmp_path / "two.vcf")
    assert cli_main([wd, "--preset", "ont", "--genotype", "--fasta", fa, "-o", one], ctx=_OracleCtx()) == 0
    made = []
    monkeypatch.setenv("CUTESV_AMD_DEVICES", "0,0")
    assert cli_main([wd, "--preset", "ont", "--genotype", "--fasta", fa, "-o", two], ctx=lambda d: made.append(d) or _OracleCtx()) == 0
    assert made == [0, 0]
    with open(one) as f1, open(two) as f2:
        a, b = f1.read(), f2.read()
    assert a == b and a.count("\n") > 10
    # ... and the stage itself: one backing behind every chromosome, rows equal to one device's
    lazy = resolve.phase3(wd, idx, Params.ont(genotype=True), devices=[0, 1], ctx=lambda d: _OracleCtx())
    assert len({id(v.backing()) for v in lazy.values()}) == 1
    assert {c: list(v) for c, v in lazy.items()} == resolve.phase3(wd, idx, Params.ont(genotype=True), ctx=_OracleCtx(), lazy=False)


def _fake_call_gt(bam, pos_1, pos_2, chr_1, chr_2, read_ids, max_cluster_bias, gt_round):
    """stands in for tra_bam.call_gt (cuteSV_resolveTRA.py:258-309 over a BAM): deterministic DR, count_coverage giving up
    for every third position"""
    from cutesv_amd.genotype import gl_fields, gl_index
    n = len(read_ids)
    if int(pos_1) % 3 == 0:
        return str(n), ".", "./.", ".,.,.", ".", "."
    dr = int(pos_1) % 7
    return (str(n), str(dr)) + tuple(gl_fields(gl_index(dr, n)))


@pytest.fixture()
def fake_bam(monkeypatch):
    import types
    from cutesv_amd import tra_bam
    fake = types.ModuleType("pysam")
    fake.AlignmentFile = lambda path: types.SimpleNamespace(close=lambda: None)
    monkeypatch.setitem(sys.modules, "pysam", fake)
    monkeypatch.setattr(tra_bam, "call_gt", _fake_call_gt)
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "bam")
    return tra_bam


def test_bam_mode_tra_genotypes_reach_the_rows_and_the_vcf(tmp_path, fake_bam, monkeypatch):
    st, p, case = _golden("realnames_gt")
    assert p.genotype
    wd = str(tmp_path / "wd") + "/"
    os.makedirs(wd)
    idx = st.write_reference_workdir(wd)
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "off")
    plain = resolve.phase3(wd, idx, p, ctx=_OracleCtx(), lazy=False)
    monkeypatch.setenv("CUTESV_AMD_TRA_GT", "bam")
    with pytest.raises(ValueError):
        resolve.phase3(wd, idx, p, ctx=_OracleCtx())                        # (bam mode needs the BAM)
    eager = resolve.phase3(wd, idx, p, bam="x.bam", ctx=_OracleCtx(), lazy=False)
    lazy = resolve.phase3(wd, idx, p, bam="x.bam", devices=[0, 0], ctx=lambda d: _OracleCtx())
    n_tra = n_gave_up = 0
    for ch, rows in plain.items():
        tra = [r for r in rows if r[1] not in ("DEL", "INS", "DUP", "INV")]
        want = [r for r in rows if r[1] in ("DEL", "INS", "DUP", "INV")] + fake_bam.genotype_rows(tra, "x.bam", p.max_cluster_bias_TRA, p.gt_round)
        assert eager[ch] == want, ch                                         # what run_tra returns for the task
        assert list(lazy[ch]) == want, ch
        n_tra += len(tra)
        n_gave_up += sum(1 for r in want[len(want) - len(tra):] if r[6] == ".")
    assert n_tra > 10 and 0 < n_gave_up < n_tra
    # the VCF body: the BND records carry the host's genotype
    fa = _write_fasta(tmp_path, st)
    out = str(tmp_path / "bam.vcf")
    assert cli_main([wd, "--genotype", "--bam", "x.bam", "--fasta", fa, "-o", out], ctx=_OracleCtx()) == 0
    want = {}
    for ch, rows in resolve.phase3(wd, idx, Params(genotype=True), bam="x.bam", ctx=_OracleCtx(), lazy=False).items():
        for r in rows:
            if r[1] not in ("DEL", "INS", "DUP", "INV"):
                pos = int(r[2]) + (0 if r[1].startswith("N") else 1)                   # (BND POS, main script / GT:400-458)
                want[(ch, pos)] = (r[7], r[6])
    seen = 0
    with open(out) as f:
        for line in f:
            x = line.rstrip("\n").split("\t")
            if "SVTYPE=BND" in x[7]:
                gt, dr = x[9].split(":")[:2]
                assert (gt, dr) == want[(x[0], int(x[1]))]
                seen += 1
    assert seen == len(want) > 10


def test_a_row_filed_under_another_chromosome_sends_the_directory_through_pickle(tmp_path):
    """a block whose rows name another chromosome than its key: from_reference_workdir's store (it goes by the rows' own field),
    for a walked block (walk_workdir reports False) and for a block pickle.load reads alike"""
    st, p, case = _golden("ont_gt")
    wd = str(tmp_path) + "/"
    idx = st.write_reference_workdir(wd)
    chs = sorted(idx["DEL"])
    for protocol in (4, 0):
        bad = _rewrite_block(wd, idx, "DEL", chs[1], _block(wd, idx, "DEL", chs[0]), protocol)    # chr A's rows filed under chr B
        mm = open(wd + "DEL.pickle", "rb").read()
        width, fi, fs, chk, key = _WALK["DEL"]
        t = cn.walk_workdir(((mm, bad["DEL"][chs[1]], -1, width, fi, fs, chk, chs[1].encode(), key),), 1)[0]
        assert t is (False if protocol == 4 else None)
        want = SigStore.from_reference_workdir(wd, bad)
        got = SigStore.from_reference_workdir_native(wd, bad)
        _assert_same_store(want, got)
        assert got.narrow and "a" in got.narrow


def test_chromosome_ranks_do_not_depend_on_reading_the_reads(tmp_path):
    """an empty reads block names no chromosome, a reads-only block names one - with or without the reads"""
    st, p, case = _golden("ont_gt")
    wd = str(tmp_path) + "/"
    idx = st.write_reference_workdir(wd)
    blk = _block(wd, idx, "reads", sorted(idx["reads"])[0])
    idx = _rewrite_block(wd, idx, "reads", "0_empty", [], 4)
    idx = _rewrite_block(wd, idx, "reads", "0_reads_only", [r[:4] + ("0_reads_only",) for r in blk[:1]], 4)
    want = SigStore.from_reference_workdir(wd, idx).chroms
    assert "0_reads_only" in want and "0_empty" not in want
    for reads in (True, False):
        assert SigStore.from_reference_workdir_native(wd, idx, reads=reads).chroms == want


# ------------------------------------------------------------------------------------------------ on the MI355X
def _run(tmp_path, *args, timeout=600):
    out = str(tmp_path / "phase3.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CUTESV_AMD_TRA_GT="off")
    for k in ("CUTESV_AMD_BROKER_NAME", "CUTESV_AMD_DEVICE", "CUTESV_AMD_DEVICES"):
        env.pop(k, None)
    subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, RUNNER, "--out", out, "--work", str(tmp_path)] + list(args),
                   check=True, env=env, timeout=timeout + 30)
    with open(out) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["cfg3_s025", "cfg4_s002", "cfg5_s002"])
def test_phase3_on_the_gpu_equals_the_reference_digests(tmp_path, cfg):
    r = _run(tmp_path, "--cfg", cfg)
    d = load_json("digests.json")[cfg]
    got = r["digests"]
    for key, (n, h) in d["segments"].items():
        if n:
            assert got[key] == [n, h], key
    assert sum(1 for v in got.values() if v[0]) == sum(1 for v in d["segments"].values() if v[0])
    # one process, the HIP library mapped, no broker socket, no child process
    assert r["mapped_hip_library"] and r["sockets"] == [] and r["children"] == []


@pytest.mark.gpu
def test_phase3_on_the_gpu_full_size_cfg3_equals_the_oracle(tmp_path):
    r = _run(tmp_path, "--cfg", "cfg3", "--oracle", timeout=900)
    assert r["digests"] == r["oracle_digests"] and len(r["digests"]) > 10
