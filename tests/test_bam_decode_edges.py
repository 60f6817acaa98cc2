"""The BAM record decode (bam.hip.h) at its tiers: the uint4 body and the tail of the CIGAR copy, the wavefront / workgroup
boundary at 4 096 operations, CG arrays on every byte alignment, the placeholder rule one condition at a time, 64-bit spans, clips,
flag classes, SA tag types and the spans of the one-workgroup scan.

Two truths: bam.decode_host, column by column (test_bam_reader._device_equals_host), and the records as they were handed to the
writer (assert_matches_stubs), which shares no code with the reader.  Whether the placeholder rule is htslib's is NOT checked here:
there is no htslib in the test environment; the rule is the SAM specification's 4.2.2 as bam.decode_host states it."""
import numpy as np
import pytest

from cutesv_amd import bam, synth
from test_bam_reader import _device_equals_host, assert_matches_stubs, _write_mixed

REFS = [("7", 2 ** 31 - 1), ("X", 156040895)]
OP_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 5003)
CG_SIZES = (1, 3, 4, 5, 64, 65, 4097)
FLAGS = (0, 16, 256, 272, 2048, 2064, 4, 1, 17, 1024, 0x900)
SA = "1,2239803,-,2063S670M3490S,0,3;"
SCAN_SIZES = (1023, 1024, 1025, 2049, 3073)


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


class Records:
    """the records as the writer takes them (`out`) and as the decode must give them back (`want`: the dicts of StubRecord)"""

    def __init__(self):
        self.out, self.want, self.pos, self.rng = [], [], 1000, np.random.RandomState(26)

    def add(self, name, cigar, tags=(), flag=0, mapq=None, cg=False, start=None, seq_len=None, want_cigar=None, want_tags=None):
        k = len(self.out)
        if start is None:
            start, self.pos = self.pos, self.pos + int(self.rng.randint(0, 300))
        if seq_len is None:
            seq_len = sum(ln for op, ln in cigar if op in (0, 1, 4, 7, 8))
        mapq = int(self.rng.randint(0, 61)) if mapq is None else mapq
        tags = list(tags)
        self.out.append(dict(name=name, flag=flag, mapq=mapq, start=start, cigar=cigar, seq=synth.pseudo_sequence(seq_len, 2600 + k), refid=0, tags=tags, cg=cg))
        self.want.append(dict(name=name, flag=flag, mapq=mapq, start=start, cigar=[list(x) for x in (cigar if want_cigar is None else want_cigar)], seq_len=seq_len, seq_key=2600 + k,
                              tags=[t for t in tags if t[0] == "SA"] if want_tags is None else want_tags))

    def varied(self, n_ops):
        """clips at the ends, then M / I / D / = / X / N in turn with random lengths: a mis-copied word shows in `cigar` and in `ref_end`"""
        ops = []
        for k in range(n_ops):
            op = 4 if k == 0 and n_ops > 1 else 5 if k == n_ops - 1 and n_ops > 2 else (0, 1, 0, 2, 7, 8, 3)[k % 7]
            ops.append((op, int(self.rng.randint(1, 40))))
        return ops


def crafted():
    R = Records()
    for n in OP_COUNTS:                                      # 4097 and 5003: two records of the long list in one chunk
        R.add("ops_%d" % n, R.varied(n), tags=[("NM", n)], flag=16 if n % 2 else 0)
    # a span beyond 2^32 out of operations of 2^28 - 1 bases
    big = 2 ** 28 - 1
    R.add("span_2_32", [(0, 10)] + [(3, big), (2, big)] * 10 + [(0, 10)], tags=[("SA", SA)])
    # CG arrays: the tag sits behind XZ:Z:<c characters>, so the array begins on every byte alignment
    for n in CG_SIZES:
        for c in range(16):
            R.add("cg_%d_%d" % (n, c), R.varied(n), tags=[("XZ", "Z", "x" * c)], cg=True)
    # the placeholder test, one condition broken at a time (l_seq = 30; the real operations are in the tag)
    real = [(4, 5), (0, 20), (2, 7), (0, 5)]
    tag = ("CG", "B", ("I", [ln << 4 | op for op, ln in real]))
    other = [(0, 15), (1, 15)]
    tag2 = ("CG", "B", ("I", [ln << 4 | op for op, ln in other]))
    R.add("ph_valid", [(4, 30), (3, 27)], tags=[tag], seq_len=30, want_cigar=real)
    R.add("ph_first_not_S", [(5, 30), (3, 27)], tags=[tag], seq_len=30)
    R.add("ph_S_len_differs", [(4, 29), (3, 27)], tags=[tag], seq_len=30)
    R.add("ph_second_not_N", [(4, 30), (2, 27)], tags=[tag], seq_len=30)
    R.add("ph_three_ops", [(4, 30), (3, 27), (0, 1)], tags=[tag], seq_len=30)
    R.add("ph_type_B_i", [(4, 30), (3, 27)], tags=[("CG", "B", ("i", [ln << 4 | op for op, ln in real]))], seq_len=30)
    R.add("ph_Z_before_BI", [(4, 30), (3, 27)], tags=[("CG", "Z", "20M"), tag], seq_len=30, want_cigar=real)
    R.add("ph_two_BI", [(4, 30), (3, 27)], tags=[tag, tag2], seq_len=30, want_cigar=real)
    R.add("ph_two_BI_swapped", [(4, 30), (3, 27)], tags=[tag2, tag], seq_len=30, want_cigar=other)
    # clips
    R.add("clip_S_only", [(4, 33)])
    R.add("clip_H_only", [(5, 33)])
    R.add("clip_HS_SH", [(5, 3), (4, 4), (0, 30), (4, 6), (5, 7)])
    R.add("clip_none", [(0, 30), (1, 4), (0, 30)])
    R.add("clip_left_only", [(4, 9), (0, 30)])
    R.add("clip_right_only", [(0, 30), (5, 9)])
    for f in FLAGS:
        R.add("flag_%d" % f, R.varied(6), flag=f)
    # tags: SA of type A and of type H are not SA:Z; 0..5 SA:Z per record
    R.add("sa_type_A", R.varied(5), tags=[("SA", "A", "x"), ("SA", SA)], want_tags=[("SA", SA)])
    R.add("sa_type_H", R.varied(5), tags=[("SA", "H", "1AE301"), ("NM", 1)], want_tags=[])
    for k in range(6):
        R.add("sa_x%d" % k, R.varied(9), tags=[("XZ", "Z", "SA:Z:decoy")] + [("SA", "X,%d,+,%dS%dM,%d,0;" % (1000 + j, j + 1, 50 + k, 10 * j)) for j in range(k)])
    # a position close to 2^31 - 1, its end beyond (last: the file is sorted)
    R.add("pos_2_31", [(0, 50), (2, 50)], start=2 ** 31 - 6, tags=[("SA", SA)])
    return R


def write(path, R, **kw):
    return _write_mixed(path, REFS, R.out, **kw)


def one_chunk(path):
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    return ch


def assert_claims(R, cols):
    """the crafted records are where the tiers are: operation counts, CG alignments, spans"""
    n_ops = np.diff(cols["cig_off"]).tolist()
    name = [w["name"] for w in R.want]
    by = dict(zip(name, range(len(name))))
    assert [n_ops[by["ops_%d" % n]] for n in OP_COUNTS] == list(OP_COUNTS)
    assert sum(1 for n in n_ops if n > 4096) == 2 + 16
    for n in CG_SIZES:
        idx = [by["cg_%d_%d" % (n, c)] for c in range(16)]
        assert sorted(int(cols["cg_beg"][i]) % 16 for i in idx) == list(range(16)), n
        assert all(n_ops[i] == n and int(cols["cg_end"][i] - cols["cg_beg"][i]) == 4 * n for i in idx)
    i = by["span_2_32"]
    assert int(cols["ref_end"][i] - cols["ref_start"][i]) == 20 * (2 ** 28 - 1) + 20 > 2 ** 32
    i = by["pos_2_31"]
    assert int(cols["ref_start"][i]) == 2 ** 31 - 6 and int(cols["ref_end"][i]) == 2 ** 31 + 94
    used_tag = {w["name"]: n_ops[by[w["name"]]] for w in R.want if w["name"].startswith("ph_")}
    assert used_tag == dict(ph_valid=4, ph_first_not_S=2, ph_S_len_differs=2, ph_second_not_N=2, ph_three_ops=3, ph_type_B_i=2, ph_Z_before_BI=4, ph_two_BI=4,
                            ph_two_BI_swapped=2)
    assert [int(cols["cg_beg"][by[k]]) >= 0 for k in ("ph_valid", "ph_type_B_i", "ph_first_not_S")] == [True, False, True]
    assert (int(cols["clip_left"][by["clip_S_only"]]), int(cols["clip_right"][by["clip_S_only"]])) == (33, 33)
    assert (int(cols["clip_left"][by["clip_H_only"]]), int(cols["clip_right"][by["clip_H_only"]])) == (33, 33)
    assert (int(cols["clip_left"][by["clip_HS_SH"]]), int(cols["clip_right"][by["clip_HS_SH"]])) == (3, 7)
    assert [int(cols["cls"][by["flag_%d" % f]]) for f in FLAGS] == [1, 1, 0, 0, 2, 2, 2, 2, 2, 2, 2]
    sa = np.diff(cols["sa_off"])
    assert [int(sa[by["sa_x%d" % k]]) for k in range(6)] == list(range(6)) and int(sa[by["sa_type_A"]]) == 1 and int(sa[by["sa_type_H"]]) == 0


def test_host_decode_of_the_crafted_records(tmp_path):
    R = crafted()
    path = str(tmp_path / "tiers.bam")
    write(path, R)
    ch = one_chunk(path)
    cols = bam.decode_host(ch)
    assert_matches_stubs([(ch, cols)], R.want)
    assert_claims(R, cols)


def scan_records(n):
    """record i: (7 i) mod 5 operations and i mod 3 SA tags - the two totals differ, so swapped columns show"""
    R = Records()
    for i in range(n):
        k = (7 * i) % 5
        ops = [(0, 10 + i % 7)] + [((1, 2, 0, 3)[j % 4], 1 + (i + j) % 9) for j in range(k - 1)] if k else []
        R.add("n%04d" % i, ops, tags=[("SA", "X,%d,-,%dS%dM,%d,1;" % (i + 1, j + 1, 40 + i % 50, j)) for j in range(i % 3)], start=1000 + 2 * i, seq_len=30, mapq=i % 61)
    return R


def test_host_decode_of_the_scan_chunks(tmp_path):
    R = scan_records(SCAN_SIZES[-1])
    path = str(tmp_path / "scan.bam")
    write(path, R)
    ch = one_chunk(path)
    assert ch.n == 3073
    assert_matches_stubs([(ch, bam.decode_host(ch))], R.want)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_decode_of_the_crafted_records(ctx, tmp_path):
    R = crafted()
    path = str(tmp_path / "tiers.bam")
    write(path, R)
    ch = one_chunk(path)
    got = _device_equals_host(ctx, ch, "tiers")
    assert_matches_stubs([(ch, got)], R.want)
    assert_claims(R, got)


@pytest.mark.gpu
def test_gpu_scan_spans(ctx, tmp_path):
    """chunks of 1 023 .. 3 073 records: a thread of the one-workgroup scan owns 1, 2, 3 and 4 records"""
    R = scan_records(SCAN_SIZES[-1])
    path = str(tmp_path / "scan.bam")
    write(path, R)
    n_ops = np.array([len(w["cigar"]) for w in R.want], np.int64)
    n_sa = np.array([len(w["tags"]) for w in R.want], np.int64)
    with bam.BamFile(path) as bf:
        for n in SCAN_SIZES:
            ch = next(iter(bf.chunks("7", chunk_records=n)))
            assert ch.n == n
            got = _device_equals_host(ctx, ch, "scan %d" % n)
            assert np.array_equal(got["cig_off"], np.concatenate([[0], np.cumsum(n_ops[:n])])), n
            assert np.array_equal(got["sa_off"], np.concatenate([[0], np.cumsum(n_sa[:n])])), n
            assert got["n_ops"] != got["n_sa"]
            if n == SCAN_SIZES[-1]:
                assert_matches_stubs([(ch, got)], R.want)
