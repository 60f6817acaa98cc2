"""The Python face of the C ABI: every prototype is bound when the library loads, every struct has one mirror (in _abi), the
library's struct sizes are checked at load, and the one capacity-negotiating call of extract.py really negotiates: batches
that overrun the first capacity guess, through the oracle (CPU) and through a Context (gpu), host arrays and pool rows.  Also
the rule of the library's device headers: each compiles as the only include of a translation unit."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, extract, rebuild, rows, vcf
from helpers import load_json, split_case_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_KEYS = ("kind", "read", "chr", "aux", "a", "b", "c", "d")
SPLIT_READS = (104, 242, 253, 293, 397, 398, 490, 537)


def _oracle():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------ binding
def test_every_prototype_is_bound_when_the_library_loads():
    """in a fresh interpreter that imports nothing but _lib: no symbol waits for another module to give it its prototype"""
    code = ("import sys; from cutesv_amd import _lib; L = _lib.lib()\n"
            "late = [m for m in ('extract', 'rebuild', 'bam', 'rows', 'vcf') if 'cutesv_amd.' + m in sys.modules]\n"
            "bad = [n for n, res, args in _lib.SYMBOLS if args is None or getattr(L, n).argtypes is None\n"
            "       or list(getattr(L, n).argtypes) != list(args) or getattr(L, n).restype is not res]\n"
            "print('late', late, 'bad', bad, 'n', len(_lib.SYMBOLS))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["late", "[]", "bad", "[]", "n", str(len(_lib.SYMBOLS))], out
    assert all(args is not None for _, _, args in _lib.SYMBOLS)


def test_one_set_of_mirrors_and_the_library_agrees_on_their_sizes():
    homes = dict(RebuildIn=rebuild, RebuildOut=rebuild, TIE_ORDER_FN=rebuild, VcfIn=vcf, RowsIn=rows, CigarIn=extract, CigarOut=extract,
                 SplitIn=extract, SplitOut=extract, SaIn=extract, SaOut=extract, ChunkC=bam, BamIn=bam, BamOut=bam)
    assert len(homes) == 14
    for name, mod in homes.items():
        assert getattr(mod, name) is getattr(_abi, name), name
    L = _lib.lib()
    for size_of, table, n in ((L.csv_struct_size, _abi.STRUCT_SIZES, 12), (L.csv_bam_struct_size, _abi.BAM_STRUCT_SIZES, 3),
                              (L.csv_sa_struct_size, _abi.SA_STRUCT_SIZES, 2)):
        assert len(table) == n
        assert [size_of(i) for i in range(n)] == [size for _, size in table]
        assert size_of(n) == -1
    assert _abi.STRUCT_SIZES[0] == ("csv_segment", _abi.SEGMENT_DTYPE.itemsize)


def test_a_struct_of_another_size_fails_the_load(monkeypatch):
    """a stale library with the same ABI number: lib() names the struct that differs"""
    name, size = _abi.SA_STRUCT_SIZES[1]
    monkeypatch.setattr(_abi, "SA_STRUCT_SIZES", [_abi.SA_STRUCT_SIZES[0], (name, size + 8)])
    monkeypatch.setattr(_lib, "_LIB", None)
    with pytest.raises(_lib.ExtensionMissing, match="csv_sa_out"):
        _lib.lib()
    assert _lib._LIB is None


# ------------------------------------------------------------------------------------ device headers stand alone
CSRC = os.path.join(ROOT, "cutesv_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the device headers: every *.hip.h that is not host code of the one translation unit (ctx.hip.h, stage_*.hip.h)
DEVICE_HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip.h") and f != "ctx.hip.h" and not f.startswith("stage_"))


def test_the_makefile_checks_the_same_device_headers():
    """`make headers` walks DEV_HDRS: the list is the directory's"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = [ln for ln in f if ln.startswith("DEV_HDRS")]
    assert len(line) == 1 and sorted(line[0].split("=", 1)[1].split()) == DEVICE_HEADERS
    assert len(DEVICE_HEADERS) == 14


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("header", DEVICE_HEADERS)
def test_a_device_header_compiles_alone(header, tmp_path):
    """a device header includes what it uses: a translation unit of that one include passes the compiler's front end"""
    tu = tmp_path / "alone.hip"
    tu.write_text('#include "%s"\n' % header)
    p = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-I", CSRC, str(tu)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


# ------------------------------------------------------------------------------------ CIGAR retry
N_READS, QUERY_LEN = 8, 7 * 200 + 3 * 20


def _cigar_batch():
    """eight reads of (200M 20I 200M 20D) x 3 + 200M: 24 INS and 24 DEL signatures, the first capacity guess is 16"""
    cig_off, cigar = extract.encode_cigars([[(0, 200), (1, 20), (0, 200), (2, 20)] * 3 + [(0, 200)]] * N_READS)
    return cig_off, cigar, 1000 + 1000 * np.arange(N_READS, dtype=np.int64)


def _assert_cigar_expected(sig):
    reads = np.repeat(np.arange(N_READS), 3)
    assert sig["n_sig_ins"] == 24 and sig["n_sig_del"] == 24 and len(sig["piece_qoff"]) == 24
    assert np.array_equal(sig["ins_read"], reads) and np.array_equal(sig["del_read"], reads)
    assert np.array_equal(sig["ins_pos"], 1000 * (reads + 1) + np.tile([200, 620, 1040], N_READS))
    assert np.array_equal(sig["del_pos"], 1000 * (reads + 1) + np.tile([400, 820, 1240], N_READS))
    assert (sig["ins_len"] == 20).all() and (sig["del_len"] == 20).all() and (sig["piece_len"] == 20).all()
    assert (sig["ins_npiece"] == 1).all() and np.array_equal(sig["ins_piece0"], np.arange(24))
    assert np.array_equal(sig["piece_qoff"], np.tile([200, 620, 1040], N_READS))
    for k, dt, _ in _abi.CIGAR_OUT:
        assert sig[k].dtype == dt, k


def test_cigar_capacity_retry_through_the_oracle():
    assert max(16, N_READS // 4) < 24
    _assert_cigar_expected(_oracle().cigar_signatures(*_cigar_batch()))


@pytest.mark.gpu
def test_cigar_capacity_retry_on_the_gpu(ctx):
    got, want = extract.cigar_signatures(ctx, *_cigar_batch()), _oracle().cigar_signatures(*_cigar_batch())
    _assert_cigar_expected(got)
    for k, _, _ in _abi.CIGAR_OUT:
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------ split retry
@pytest.fixture(scope="module")
def split_batch():
    """case `mixture` of split_sigs.json.gz cut to eight reads that yield 27 candidates (first guess: 16) -> (encoded reads,
    their query lengths, keywords, the whole case's candidates restricted to them with `read` renumbered)"""
    case = next(c for c in load_json("split_sigs.json.gz") if c["name"] == "mixture")
    enc_all, _, _, _, kw = split_case_inputs(case)
    whole = _oracle().split_signatures(enc_all, **kw)
    keep = np.isin(whole["read"], SPLIT_READS)
    want = {k: whole[k][keep] for k in SPLIT_KEYS}
    want["read"] = np.searchsorted(SPLIT_READS, want["read"]).astype(np.int32)
    enc, _, queries, _, _ = split_case_inputs(dict(case, reads=[case["reads"][i] for i in SPLIT_READS]))
    return enc, [len(q) for q in queries], kw, want


def _assert_split_expected(got, want):
    assert len(want["kind"]) == 27 > max(16, 2 * len(SPLIT_READS))
    for k in SPLIT_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_split_capacity_retry_through_the_oracle(split_batch):
    enc, _, kw, want = split_batch
    _assert_split_expected(_oracle().split_signatures(enc, **kw), want)


@pytest.mark.gpu
def test_split_capacity_retry_on_the_gpu(ctx, split_batch):
    enc, _, kw, want = split_batch
    _assert_split_expected(extract.split_signatures(ctx, enc, **kw), want)


# ------------------------------------------------------------------------------------ pool attach, both paths
@pytest.mark.gpu
def test_pool_attach_of_the_cigar_scan_and_of_the_split_analysis(ctx, split_batch):
    rebuild.pool_reset(ctx)
    base = rebuild.pool_rows(ctx)
    sig = extract.cigar_signatures(ctx, *_cigar_batch(), pool=dict(seg_ins=0, seg_del=1, read_base=5, query_len=np.full(N_READS, QUERY_LEN, np.int32)),
                                   host_outputs=False)
    assert all(len(sig[k]) == 0 and sig[k].dtype == dt for k, dt, _ in _abi.CIGAR_OUT)
    assert sig["n_sig_ins"] == 24 and sig["n_sig_del"] == 24
    assert rebuild.pool_rows(ctx) == base + 48
    enc, qlen, kw, _ = split_batch
    ssig = extract.split_signatures(ctx, enc, pool=dict(seg_base=[0, 8, 16, 24, 32], read_base=5, query_len=qlen), host_outputs=False, **kw)
    assert all(len(ssig[k]) == 0 for k in SPLIT_KEYS)
    assert ssig["n"] == 27
    assert rebuild.pool_rows(ctx) == base + 48 + 27
    rebuild.pool_reset(ctx)
