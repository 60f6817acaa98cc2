"""A BGZF-compressed reference FASTA (cutesv_amd/fasta.py BgzfReference, cutesv_amd/csrc/ref_core.h, k_ref_gather at the end of
bam.hip.h, stage_ref.hip.h, csv_vcf_ref_ranges / csv_vcf_emit_ref and csv_fasta_index_stream in vcf_emit.cpp).

CPU: the .gzi against an independent writer (tests/gzi_writer.py) and its refusals; open_reference by content; fetch against the
plain twin around every line and block boundary; the streamed .fai against csv_fasta_index at every cut; ranges + host gather +
csv_vcf_emit_ref against csv_vcf_emit on the golden VCF cases; the gather core's host form under the address and undefined-behaviour
sanitizers in a stand-alone program (tests/ref_core_main.cpp) against the library's.
GPU (-m gpu): csv_ref_gather against csv_ref_gather_host byte for byte on crafted blocks - lengths and starts around the tile, the
line and the wavefront, offsets beyond 2^32, block layouts; capacity, refusals, damaged blocks, isolation; call_bam and the command
line with ref.fa.gz against ref.fa; k_fai_events' rows against the host form's, the .fai built through them, the overflow window.

The twin everything on the device is compared with is csv_ref_gather_host, which the CPU tests pin to plain slices of the sequence."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from cutesv_amd import _abi, _lib, bam, call, cli, extract, fasta, rebuild, synth, vcf
from cutesv_amd.columns import Params
from helpers import load_json, store_from_json
import bam_writer
import call_helpers
import gzi_writer
import ref_helpers as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("csv_ref_gather", "csv_ref_gather_host", "csv_vcf_ref_ranges", "csv_vcf_emit_ref", "csv_fasta_index_stream_open", "csv_fasta_index_stream_feed",
               "csv_fasta_index_stream_finish", "csv_fasta_index_stream_close", "csv_fasta_index_stream_carry", "csv_fasta_index_stream_rows", "csv_fai_events",
               "csv_fai_events_host")


@pytest.fixture(scope="module")
def ctx():
    from cutesv_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def test_the_new_entries_are_bound_and_the_abi_stays_9():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert all(s in names for s in NEW_SYMBOLS) and all(hasattr(_lib.lib(), s) for s in NEW_SYMBOLS)
    assert _abi.ABI_VERSION == 9 and _lib.lib().csv_abi_version() == 9
    assert fasta.DEFAULT_REF_ROUTE == "host" and fasta.REF_ROUTES == ("host", "device") and fasta.WINDOW_BLOCKS == 4096
    with open(os.path.join(ROOT, "cutesv_amd", "csrc", "ref_core.h")) as f:
        assert re.search(r"constexpr int REF_TILE = %d;" % rh.TILE, f.read())


# ------------------------------------------------------------------------------------------------ .gzi
def _pieces(n_blocks, empty_at=None):
    text = b">c\n" + b"".join(rh.bases(60, 7 + i) + b"\n" for i in range(max(1, n_blocks * 5)))
    cut = -(-len(text) // n_blocks)
    pieces = rh.cut_text(text, cut)
    assert len(pieces) == n_blocks
    if empty_at is not None:
        pieces.insert(empty_at, b"")
    return text, pieces


@pytest.mark.parametrize("n_blocks,empty_at", [(1, None), (2, None), (300, None), (5, 2)])
def test_gzi_parse_build_and_write_agree_with_the_independent_writer(tmp_path, n_blocks, empty_at):
    text, pieces = _pieces(n_blocks, empty_at)
    image = rh.bgzf_image(pieces)
    want = gzi_writer.gzi_bytes(image)
    n_all = len(pieces) + 1                                                  # the end-of-file block has its entry
    assert struct.unpack_from("<Q", want)[0] == n_all - 1 and len(want) == 8 + 16 * (n_all - 1)
    gz = str(tmp_path / "r.fa.gz")
    with open(gz, "wb") as f:
        f.write(image)
    built = fasta.BgzfReference(gz, write_gzi=True)                           # no .gzi: built by hopping headers, then written
    assert built.gzi_built and built.n_blocks == n_all and built.size == len(text)
    with open(gz + ".gzi", "rb") as f:
        assert f.read() == want
    co, uo = fasta.parse_gzi(want)
    assert co.tolist() == built.coff[1:-1].tolist() and uo.tolist() == built.uoff[1:-1].tolist()
    assert fasta.gzi_bytes(built.coff[:-1], built.uoff[:-1]) == want
    if empty_at is not None:
        assert built.uoff[empty_at] == built.uoff[empty_at + 1]
    read = fasta.BgzfReference(gz)                                            # through the file this time
    assert not read.gzi_built and read.coff.tolist() == built.coff.tolist() and read.uoff.tolist() == built.uoff.tolist()
    assert read.fetch("c") == text[3:].replace(b"\n", b"").decode() == built.fetch("c")
    assert not os.path.exists(gz + ".fai")
    # a .gzi that stops short of the end-of-file block's entry describes the same file
    with open(gz + ".gzi", "wb") as f:
        f.write(struct.pack("<Q", n_all - 2) + want[8:-16])
    assert fasta.BgzfReference(gz).coff.tolist() == built.coff.tolist()
    built.close(); read.close()


def _age(path, seconds):
    t = os.path.getmtime(path) - seconds
    os.utime(path, (t, t))


def test_a_stale_gzi_is_rebuilt_and_a_stale_fai_too(tmp_path):
    text, pieces = _pieces(4)
    gz = str(tmp_path / "r.fa.gz")
    with open(gz, "wb") as f:
        f.write(rh.bgzf_image(pieces))
    with open(gz + ".gzi", "wb") as f:
        f.write(struct.pack("<QQQ", 1, 5, 5))                                 # (what would be refused, were it read)
    with open(gz + ".fai", "w") as f:
        f.write("zzz\t5\t3\t60\t61\n")
    _age(gz + ".gzi", 100); _age(gz + ".fai", 100)
    ref = fasta.BgzfReference(gz)
    assert ref.gzi_built and ref.fai_built and ref.names == ["c"] and ref.n_blocks == 5


def test_gzi_refusals_name_the_file(tmp_path):
    text, pieces = _pieces(4)
    image = rh.bgzf_image(pieces)
    gz = str(tmp_path / "r.fa.gz")
    good = gzi_writer.gzi_bytes(image)
    co, uo = fasta.parse_gzi(good)

    def put(gzi):
        for name, data in ((gz, image), (gz + ".gzi", gzi), (gz + ".fai", b"c\t1200\t3\t60\t61\n")):       # (a .fai: nothing is inflated before a fetch)
            with open(name, "wb") as f:
                f.write(data)

    def pairs(c, u):
        return struct.pack("<Q", len(c)) + b"".join(struct.pack("<QQ", int(a), int(b)) for a, b in zip(c, u))
    put(pairs([co[1], co[0], co[2]], uo[:3]))
    with pytest.raises(fasta.BgzfReferenceError, match=r"r\.fa\.gz\.gzi does not describe .*r\.fa\.gz \(offsets that do not increase\)"):
        fasta.BgzfReference(gz)
    put(pairs(co[:2], [uo[1], uo[0]]))
    with pytest.raises(fasta.BgzfReferenceError, match="offsets that do not increase"):
        fasta.BgzfReference(gz)
    put(pairs(list(co[:2]) + [len(image) + 5], list(uo[:2]) + [uo[1] + 9]))
    with pytest.raises(fasta.BgzfReferenceError, match=r"r\.fa\.gz\.gzi does not describe .* \(an offset beyond the file\)"):
        fasta.BgzfReference(gz)
    put(good[:-3])
    with pytest.raises(fasta.BgzfReferenceError, match=r"r\.fa\.gz\.gzi says 4 entries"):
        fasta.BgzfReference(gz)
    # a touched block whose header is not a BGZF header at that offset: the table is off by three bytes for block 2
    c2 = co.copy(); c2[1] += 3
    put(pairs(c2, uo))
    ref = fasta.BgzfReference(gz)
    assert not ref.gzi_built and not ref.fai_built
    assert ref.fetch("c", 0, 5) == text[3:8].decode()                         # (block 0 is as the table says: untouched blocks are not looked at)
    in2 = (int(uo[1]) + 70 - 3) // 61 * 60                                      # a base whose line lies in block 2
    with pytest.raises(fasta.BgzfReferenceError, match=r"r\.fa\.gz: no BGZF block header at byte %d" % c2[1]):
        ref.fetch("c", in2, in2 + 5)
    # a touched block whose ISIZE is not the difference of the table's uncompressed offsets
    u2 = uo.copy(); u2[1] += 1
    put(pairs(co, u2))
    ref = fasta.BgzfReference(gz)
    assert ref.fetch("c", 0, 5) == text[3:8].decode()
    with pytest.raises(fasta.BgzfReferenceError, match=r"r\.fa\.gz: the BGZF block at byte %d says ISIZE %d, the block table says %d" % (co[0], uo[1] - uo[0], uo[1] - uo[0] + 1)):
        ref.fetch("c")


# ------------------------------------------------------------------------------------------------ open_reference
def test_open_reference_decides_by_content(tmp_path):
    import gzip
    text, seqs = rh.crafted_fasta(big=False)
    plain, gz, image = rh.write_pair(tmp_path, text, 300)
    odd = str(tmp_path / "reference.bin")                                     # BGZF under a name without .gz
    shutil.copy(gz, odd)
    ref = fasta.open_reference(odd)
    assert isinstance(ref, fasta.BgzfReference) and ref.names == list(seqs) and ref.fetch("lb60") == seqs["lb60"] and "lb61" in ref and "nope" not in ref
    assert isinstance(fasta.open_reference(plain), fasta.Reference)
    plain_gz = str(tmp_path / "plain.fa.gz")
    with gzip.open(plain_gz, "wb") as f:
        f.write(text)
    with pytest.raises(ValueError, match="must be compressed with bgzip"):
        fasta.open_reference(plain_gz)
    with pytest.raises(ValueError, match="cannot be memory-mapped"):            # as before
        fasta.Reference(gz)
    with pytest.raises(ValueError, match="route"):
        fasta.open_reference(gz, route="gpu")
    assert cli.split_own(["a", "--ref_route", "device", "b"])[0].ref_route == "device" and cli.split_own(["a", "b"])[0].ref_route is None
    assert cli.split_own(["a", "--ref_route", "host", "-s", "3"])[1] == ["a", "-s", "3"]
    with pytest.raises(ValueError, match="ref_route"):
        call.call_bam("no.bam", {}, Params(), ref_route="gpu")


# ------------------------------------------------------------------------------------------------ fetch
def _boundaries(ref, i):
    """contig-base indices around every line start of contig i (its first 8 lines) and its end"""
    n, lb = int(ref.length[i]), max(int(ref.line_bases[i]), 1)
    pts = {0, 1, n - 1, n, n + 3}
    for ln in range(0, min(n // lb + 1, 8)):
        pts |= {ln * lb - 1, ln * lb, ln * lb + 1}
    return sorted(p for p in pts if 0 <= p <= n + 3)


def _text_cuts(text):
    """block cuts (offsets) that separate a base from its line break, '\\r' from '\\n', and '>' from the name behind it"""
    cuts = []
    for m in re.finditer(rb"\r?\n", text):
        cuts += [m.start(), m.end() - 1]
    cuts += [m.start() + 1 for m in re.finditer(rb">", text)]
    return sorted(set(cuts))


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_fetch_equals_the_plain_twin_around_every_line_and_block_boundary(tmp_path, nl):
    big, big_seqs = rh.crafted_fasta(nl)
    small, small_seqs = rh.crafted_fasta(nl, big=False)
    fine = _text_cuts(big[:4000]) + list(range(4000, len(big), 60000))                                              # around every line break and behind every '>' of the short contigs
    for j, (text, seqs, cut) in enumerate(((small, small_seqs, 1), (big, big_seqs, fine), (small, small_seqs, 59), (small, small_seqs, 60), (small, small_seqs, 61),
                                           (small, small_seqs, 62), (big, big_seqs, 65280))):
        d = tmp_path / ("c%d" % j)
        d.mkdir()
        plain, gz, image = rh.write_pair(d, text, cut)
        want, got = fasta.Reference(plain), fasta.BgzfReference(gz)
        assert got.size == len(text) and got.fai_built and got.gzi_built
        assert got.fai_text() == "".join("%s\t%d\t%d\t%d\t%d\n" % (n, want.length[i], want.offset[i], want.line_bases[i], want.line_width[i]) for i, n in enumerate(want.names))
        assert got.names == list(seqs) and got.length.tolist() == [len(s) for s in seqs.values()]
        for i, name in enumerate(want.names):
            pts = _boundaries(want, i)
            if j > 1:
                pts = pts[:9] + pts[-5:]
            for a in pts:
                for b in pts[::3] + [pts[-1]]:
                    assert got.fetch(name, a, b) == want.fetch(name, a, b) == seqs[name][a:max(a, b)], (cut if isinstance(cut, int) else "fine", name, a, b)
            assert got.fetch(name) == seqs[name]
        # gather: the same through the core's host form, all boundaries of a contig in one call, unsorted
        for i in (0, 3, len(want.names) - 3):
            pts = np.array([p for p in _boundaries(want, i) if p <= int(want.length[i])], np.int64)
            beg = np.repeat(pts, len(pts)); end = np.tile(pts, len(pts))
            keep = end >= beg
            beg, end = beg[keep][::-1], end[keep][::-1]
            blob, off = got.gather(np.full(len(beg), i), beg, end)
            assert blob.tobytes() == rh.truth(seqs[want.names[i]].encode(), beg, end).tobytes() and off.tolist() == np.concatenate([[0], np.cumsum(end - beg)]).tolist()
        with pytest.raises(ValueError, match="does not lie inside contig"):
            got.gather([0], [0], [int(want.length[0]) + 1])
        want.close(); got.close()


def test_gather_cuts_its_windows_between_ranges(tmp_path):
    text, seqs = rh.crafted_fasta(big=False)
    plain, gz, _ = rh.write_pair(tmp_path, text, 61)
    ref = fasta.BgzfReference(gz, window_blocks=3)
    rng = np.random.default_rng(3)
    ci = rng.integers(0, len(ref.names), 200)
    beg = np.array([rng.integers(0, int(ref.length[c]) + 1) for c in ci])
    end = np.array([rng.integers(b, int(ref.length[c]) + 1) for b, c in zip(beg, ci)])
    blob, off = ref.gather(ci, beg, end)
    assert blob.tobytes().decode() == "".join(seqs[ref.names[c]][b:e] for c, b, e in zip(ci, beg, end))
    assert ref.stats["windows_host"] > 50 and ref.stats["windows_device"] == 0
    with pytest.raises(ValueError, match="needs a context"):
        ref.gather(ci, beg, end, route="device")
    assert ref.gather([], [], [])[1].tolist() == [0]


def test_a_range_wider_than_a_window_does_not_shorten_the_windows_behind_it(tmp_path):
    text, pieces = _pieces(40)
    gz = str(tmp_path / "r.fa.gz")
    with open(gz, "wb") as f:
        f.write(rh.bgzf_image(pieces))
    ref = fasta.BgzfReference(gz, window_blocks=4)
    n = int(ref.length[0])
    seq = ref.fetch("c")
    # one range across 20 blocks, then single bases in every block behind its first: 1 window for the wide range, then 4 blocks a window
    beg = np.concatenate([[10], np.arange(400, n, 97)])
    end = np.concatenate([[n // 2], np.arange(400, n, 97) + 1])
    before = ref.stats["windows_host"]
    blob, off = ref.gather(np.zeros(len(beg), np.int64), beg, end)
    assert blob.tobytes().decode() == "".join(seq[b:e] for b, e in zip(beg, end))
    assert ref.stats["windows_host"] - before <= 1 + -(-ref.n_blocks // 4) + 1
    ref.close()


# ------------------------------------------------------------------------------------------------ the streamed .fai
STREAM_TEXTS = [
    b">a d\nACGT\nACGT\nAC\n>b\nAC\n", b">a\r\nACGT\r\nAC\r\n>b x\r\n", b">a\nACGT\nAC", b">a\nACGT\n\n>b\n\nAC\n", b">a\nAC\n>b", b">a\n", b">a", b"", b"\n\r\n>a\nA\n",
    b">a\tb\rc\nAC\n", b"AC", b"\n>a\nACG\nAC\n\n", b">a\nAC\r\nAC\n", b">a\nACGT\nAC\nA\n>b\nAA\n",
    # refused
    b"AC\n>a\nAC\n", b">a\nAC\nACGT\n", b">a\nACGT\nAC\nACGT\n", b">a\nAC\n\nAC\n", b">a\nACGT\nAC\nAC\n", b"x\n",
]


def _index_whole(text):
    cap = 16
    a = [np.zeros(cap, dt) for dt in (np.int64, np.int32, np.int64, np.int64, np.int32, np.int32)]
    buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
    n = _lib.lib().csv_fasta_index(C.c_void_p(buf.ctypes.data), len(text), cap, *[x.ctypes.data for x in a])
    if n < 0:
        return int(n)
    return [(text[int(a[0][i]):int(a[0][i]) + int(a[1][i])], int(a[2][i]), int(a[3][i]), int(a[4][i]), int(a[5][i])) for i in range(n)]


def _index_stream(windows):
    L = _lib.lib()
    h = L.csv_fasta_index_stream_open()
    try:
        for w in windows:
            b = np.frombuffer(w, np.uint8) if w else np.zeros(0, np.uint8)
            L.csv_fasta_index_stream_feed(h, b.ctypes.data if len(b) else None, len(b))
        cap = 16
        a = [np.zeros(cap, dt) for dt in (np.int64, np.int32, np.int64, np.int64, np.int32, np.int32)]
        names, nb = np.zeros(256, np.uint8), C.c_int64(0)
        n = L.csv_fasta_index_stream_finish(h, cap, names.ctypes.data, len(names), C.byref(nb), *[x.ctypes.data for x in a])
        again = L.csv_fasta_index_stream_finish(h, 0, None, 0, None, None, None, None, None, None, None)
        assert again == n
        if n < 0:
            return int(n)
        return [(names[int(a[0][i]):int(a[0][i]) + int(a[1][i])].tobytes(), int(a[2][i]), int(a[3][i]), int(a[4][i]), int(a[5][i])) for i in range(n)]
    finally:
        L.csv_fasta_index_stream_close(h)


def test_the_streamed_index_equals_the_whole_one_at_every_cut():
    refused = 0
    for text in STREAM_TEXTS:
        want = _index_whole(text)
        refused += want == -_abi.E_INVALID
        assert _index_stream([text]) == want, text
        assert _index_stream([text[i:i + 1] for i in range(len(text))]) == want, text
        for cut in range(len(text) + 1):
            assert _index_stream([text[:cut], text[cut:]]) == want, (text, cut)
            assert _index_stream([text[:cut], b"", text[cut:cut + 2], text[cut + 2:]]) == want, (text, cut)
    assert 6 <= refused <= len(STREAM_TEXTS) - 10                             # (csv_fasta_index is the judge: both verdicts occur)
    for nl in (b"\n", b"\r\n"):
        text, _ = rh.crafted_fasta(nl, big=False)
        want = _index_whole(text)
        assert isinstance(want, list) and len(want) == 11
        for step in (1, 7, 61, 64, 1000):
            assert _index_stream(rh.cut_text(text, step)) == want


def test_faidx_command_line_writes_what_the_plain_twin_has(tmp_path, capsys):
    text, seqs = rh.crafted_fasta(big=False)
    plain, gz, image = rh.write_pair(tmp_path, text, 777)
    want = fasta.Reference(plain, write_fai=True)
    with open(plain + ".fai") as f:
        fai = f.read()
    assert fasta.main([gz, "--faidx"]) == 0
    assert capsys.readouterr().out == fai and not os.path.exists(gz + ".fai") and not os.path.exists(gz + ".gzi")
    assert fasta.main([gz, "--faidx", "--write"]) == 0
    with open(gz + ".fai") as f:
        assert f.read() == fai
    with open(gz + ".gzi", "rb") as f:
        assert f.read() == gzi_writer.gzi_bytes(image)
    ref = fasta.BgzfReference(gz)
    assert not ref.fai_built and not ref.gzi_built and ref.fetch("lb61", 3, 200) == seqs["lb61"][3:200]
    # a .fai that points beyond the text is refused under Reference's rule, against the uncompressed size
    with open(gz + ".fai", "w") as f:
        f.write("x\t%d\t3\t60\t61\n" % len(text))
    with pytest.raises(ValueError, match="offsets beyond the file"):
        fasta.BgzfReference(gz)
    os.remove(plain + ".fai")
    assert fasta.main([plain, "--faidx"]) == 0 and capsys.readouterr().out == fai
    want.close()


# ------------------------------------------------------------------------------------------------ the emitter
def _write_fasta(path, seqs, width):
    with open(path, "w") as f:
        for name, s in seqs.items():
            f.write(">%s d\n" % name + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)))


def test_ranges_host_gather_and_emit_ref_give_the_emitters_text(tmp_path):
    small = {c["name"]: c for c in load_json("small_cases.json.gz")}
    golden = load_json("vcf_lines.json.gz")
    done, kinds = 0, set()
    for k, g in enumerate(golden):
        case = small[g["case"]]
        st = store_from_json(case["store"])
        p = Params(**case["params"])
        ref = {c: synth.reference_sequence(g["ref_len"], seed=g["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
        d = tmp_path / ("g%d" % k)
        d.mkdir()
        _write_fasta(str(d / "ref.fa"), ref, 60 if k % 2 == 0 else 17)
        with open(str(d / "ref.fa"), "rb") as f:
            text = f.read()
        _, gz, _ = rh.write_pair(d, text, 65280 if k % 3 else 4001)
        zref = fasta.open_reference(gz)
        from oracle import oracle
        hb = st.host_batch([(t, c) for t, c, _ in case["rows"]], p)
        res = oracle.cluster_batch(hb, per_sig=False)
        for max_size in (p.max_size, -1):
            kw = dict(min_size=p.min_size, max_size=max_size, genotype=p.genotype, **g["flags"])
            want, sv_want = vcf.emit_records(st, hb.segments, res, ref, **kw)
            got, sv_got = vcf.emit_records(st, hb.segments, res, zref, **kw)
            assert got == want and sv_got.tolist() == sv_want.tolist(), (g["case"], g["flags"], max_size)
            kinds |= {(bool(g["flags"].get("ignore_sequence")), bool(g["flags"].get("report_readid")), bool(p.genotype))}
        done += 1
    assert done >= 21 and len(kinds) >= 4 and zref.stats["windows_host"] > 0


@pytest.fixture(scope="module")
def tra_case():
    from oracle import oracle
    case = load_json("tra_genotype.json.gz")[0]
    st = store_from_json(case["store"])
    p = Params(**case["params"])
    ref = {c: synth.reference_sequence(int(st.contig_len[i]), seed=case["vcf"]["ref_seed0"] + i) for i, c in enumerate(st.chroms)}
    hb = st.host_batch([(t, c) for t, c, _ in case["rows"]], p)
    return st, p, ref, hb, oracle.cluster_batch(hb, per_sig=False)


def test_a_contig_missing_from_the_fasta_and_the_capacity_retry(tmp_path, tra_case, monkeypatch):
    st, p, ref, hb, res = tra_case
    kw = dict(min_size=p.min_size, max_size=p.max_size, genotype=True, report_readid=True)
    _write_fasta(str(tmp_path / "ref.fa"), ref, 60)
    with open(str(tmp_path / "ref.fa"), "rb") as f:
        _, gz, _ = rh.write_pair(tmp_path, f.read(), 65280)
    want, _ = vcf.emit_records(st, hb.segments, res, ref, **kw)
    assert vcf.emit_records(st, hb.segments, res, fasta.open_reference(gz), **kw)[0] == want and "SVTYPE=BND" in want
    # BND calls on a contig the FASTA does not have say 'N'; the text is the one the dictionary without that contig gives
    for drop in st.chroms:
        part = {c: s for c, s in ref.items() if c != drop}
        d = tmp_path / ("without_" + drop)
        d.mkdir()
        _write_fasta(str(d / "ref.fa"), part, 60)
        with open(str(d / "ref.fa"), "rb") as f:
            _, gz2, _ = rh.write_pair(d, f.read(), 65280)
        try:
            want2 = vcf.emit_records(st, hb.segments, res, part, **kw)[0]
        except RuntimeError as e:
            with pytest.raises(RuntimeError, match=re.escape(str(e))):           # the others -> the same error
                vcf.emit_records(st, hb.segments, res, fasta.open_reference(gz2), **kw)
            continue
        assert vcf.emit_records(st, hb.segments, res, fasta.open_reference(gz2), **kw)[0] == want2
        assert want2 != want and "\tN\t" in want2
    # the capacity retry: the first call sees a buffer one byte short of the text
    real, seen = _lib.lib(), []

    class Short:
        def __getattr__(self, name):
            return getattr(real, name)

        def csv_vcf_emit_ref(self, vin, blob, off, out, cap, need, sv):
            short = len(want.encode()) - 1 if not seen else cap
            rc = real.csv_vcf_emit_ref(vin, blob, off, out, short, need, sv)
            seen.append((rc, short, need._obj.value))
            return rc
    monkeypatch.setattr(vcf, "lib", lambda: Short())
    got = vcf.emit_records(st, hb.segments, res, fasta.open_reference(gz), **kw)[0]
    monkeypatch.undo()
    n = len(want.encode())
    assert got == want and [x[0] for x in seen] == [_abi.E_CAPACITY, _abi.OK] and seen[0][1:] == (n - 1, n) and seen[1][2] == n


# ------------------------------------------------------------------------------------------------ the core: host form, sanitizers
def _core_cases():
    """[(name, blocks [(uoff, bytes)], Ranges, sequence or None)]: what the CPU pins to plain slices and the GPU to the host form"""
    out = []
    for j, lb in enumerate((1, 2, 59, 60, 61, 63, 64, 65, 4096, None)):
        for gap in (1, 2):
            n = 9000 if lb not in (4096, None) else 3 * 4096 + 77
            seq = rh.bases(n, 40 + j)
            text, base_off, lw = rh.line_layout(seq, lb, gap)
            beg, end = rh.range_set(n, lb or n, lens_big=(rh.TILE - 1, rh.TILE, rh.TILE + 1))
            out.append(("lb %s gap %d" % (lb, gap), rh.blocks_at(text, 1000 + 37 * j), rh.Ranges(base_off, lb or n, lw, beg, end), seq))
    return out


def test_the_host_form_gives_plain_slices():
    for name, blocks, R, seq in _core_cases():
        rc, got, out_off, need, err, _ = rh.gather_host(rh.Blocks(blocks), R)
        assert rc == _abi.OK and err == "", (name, err)
        assert got.tobytes() == rh.truth(seq, R.beg, R.end).tobytes(), name
        assert out_off.tolist() == np.concatenate([[0], np.cumsum(R.end - R.beg)]).tolist() and need == out_off[-1]


def test_the_core_under_the_sanitizers_gives_the_same_bytes(tmp_path):
    """ref_core.h's host form - the code the wavefronts run, with one lane - in a stand-alone program built with
    -fsanitize=address,undefined: the blocks' bytes and the output are heap blocks of exactly their size.  Ranges that leave the
    blocks are in the corpus too: the coverage test must name them, and nothing is gathered for them."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (the library's own build needs it too)"
    exe = str(tmp_path / "ref_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "ref_core_main.cpp")], check=True, capture_output=True, text=True)
    cases = _core_cases()
    # blocks that are not adjacent, with an empty one among them; ranges that read the hole, the byte in front and the byte behind
    seq = rh.bases(5000, 5)
    text, base_off, lw = rh.line_layout(seq, 60, 1)
    blocks = rh.blocks_at(text, 700)
    holed = blocks[:2] + [(blocks[2][0], b"")] + blocks[3:5] + [(blocks[5][0], b"")] + blocks[5:]
    beg = np.array([0, 600, 1300, 1500, 2000, 4999, 0, 5000], np.int64)
    end = np.array([600, 1400, 1370, 2100, 2000, 5000, 5001, 5060], np.int64)
    cases.append(("holes", holed, rh.Ranges(base_off, 60, lw, beg, end), None))
    for name, blocks, R, _ in cases:
        path, out = str(tmp_path / "corpus.bin"), str(tmp_path / "out.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(blocks)))
            for u, d in blocks:
                f.write(struct.pack("<qI", u, len(d)) + d)
            f.write(struct.pack("<I", R.n))
            for r in range(R.n):
                f.write(struct.pack("<qiiqq", R.base_off[r], R.lb[r], R.lw[r], R.beg[r], R.end[r]))
        p = subprocess.run([exe, path, out], capture_output=True, text=True)
        assert p.returncode == 0, (name, p.stderr[-3000:])
        lines = p.stdout.splitlines()
        assert lines[0] == "tile %d" % rh.TILE
        rows = np.array([[int(x) for x in ln.split()] for ln in lines[1:]], np.int64).reshape(-1, 3)
        covered = rows[:, 1].astype(bool)
        B = rh.Blocks(blocks)
        if name == "holes":
            assert covered.tolist() == [True, False, True, False, True, True, False, False]
            rc, _, out_off, need, err, guard = rh.gather_host(B, R, guard=64)
            assert rc == _abi.E_INVALID and "range 1 reads bytes that lie in none of the 9 blocks" in err and (out_off == -7).all() and need == -7 and (guard == 0xA5).all()
        else:
            assert covered.all()
        keep = rh.Ranges(R.base_off[covered], R.lb[covered], R.lw[covered], R.beg[covered], R.end[covered])
        rc, want, _, _, err, _ = rh.gather_host(B, keep)
        assert rc == _abi.OK, err
        with open(out, "rb") as f:
            assert f.read() == want.tobytes(), name
        assert rows[covered, 2].tolist() == (keep.end - keep.beg).tolist() and (rows[~covered, 2] == 0).all()


def _refusals(seq_n=500):
    """name -> (blocks, Ranges, the text the refusal must contain)"""
    seq = rh.bases(seq_n, 1)
    text, base_off, lw = rh.line_layout(seq, 60, 1)
    blocks = rh.blocks_at(text, 200)
    ok = lambda **k: rh.Ranges(k.get("base_off", base_off), k.get("lb", 60), k.get("lw", lw), k.get("beg", [0, 10]), k.get("end", [5, 20]))     # noqa: E731
    return {
        "lb 0": (blocks, ok(lb=0), "line_bases of range 0 is 0"),
        "lw below lb": (blocks, ok(lw=59), "line_width of range 0 is below its line_bases"),
        "beg below 0": (blocks, ok(beg=[0, -1]), "range 1 has beg -1 below 0"),
        "end below beg": (blocks, ok(beg=[7, 10]), "range 0 has beg 7 below 0 or beyond its end"),
        "unsorted blocks": ([blocks[1], blocks[0], blocks[2]], ok(), "blocks 0 and 1 overlap or are not sorted"),
        "overlapping blocks": ([blocks[0], (blocks[1][0] - 1, blocks[1][1])] + blocks[2:], ok(), "blocks 0 and 1 overlap"),
        "uncovered": (blocks[1:], ok(), "range 0 reads bytes that lie in none of the 2 blocks"),
        "beyond the blocks": (blocks, ok(end=[5, seq_n + 100]), "range 1 reads bytes that lie in none of the 3 blocks"),
    }


def test_the_host_entry_refuses_what_the_device_entry_refuses():
    for name, (blocks, R, why) in _refusals().items():
        rc, got, out_off, need, err, guard = rh.gather_host(rh.Blocks(blocks), R, cap=64, guard=64)
        assert rc == _abi.E_INVALID and why in err and err.startswith("csv_ref_gather_host: "), (name, err)
        assert (out_off == -7).all() and need == -7 and (guard == 0xA5).all() and len(got) == 0, name
    L = _lib.lib()
    assert L.csv_ref_gather_host(None, 0, 0, None, None, None, 0, None, None, None, None, None, None, 0, None, None, None, 0) == _abi.E_INVALID
    assert L.csv_ref_gather_host(None, 0, -1, None, None, None, 0, None, None, None, None, None, None, 0, np.zeros(1, np.int64).ctypes.data, C.byref(C.c_int64()), None, 0) == _abi.E_INVALID
    need, off = C.c_int64(-7), np.full(1, -7, np.int64)
    assert L.csv_ref_gather_host(None, 0, 0, None, None, None, 0, None, None, None, None, None, None, 0, off.ctypes.data, C.byref(need), None, 0) == _abi.OK
    assert need.value == 0 and off.tolist() == [0]


# ------------------------------------------------------------------------------------------------ GPU 1: the gather against its twin
def _device_equals_host(ctx, blocks, R, name):
    B = rh.Blocks(blocks)
    rc, want, want_off, need, err, _ = rh.gather_host(B, R)
    assert rc == _abi.OK, (name, err)
    rc, got, out_off, need_d, text, guard, status, ms = rh.gather_device(ctx, B, R, guard=64)
    assert rc == _abi.OK, (name, text)
    assert need_d == need and out_off.tolist() == want_off.tolist() and (guard == 0xA5).all() and not status.any(), name
    assert got.tobytes() == want.tobytes(), name
    return want, ms


@pytest.mark.gpu
def test_gpu_gather_equals_the_host_form_on_crafted_blocks(ctx):
    for name, blocks, R, seq in _core_cases():
        want, _ = _device_equals_host(ctx, blocks, R, name)
        assert want.tobytes() == rh.truth(seq, R.beg, R.end).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("lb,gap", [(1, 1), (60, 1), (61, 2), (64, 1), (4096, 2), (70000, 1), (None, 1)])
def test_gpu_gather_of_long_ranges(ctx, lb, gap):
    """lengths around 65536 and 200001 bases - several tiles, four or more blocks - at the starts around a line's ends"""
    n = 270_000
    seq = rh.bases(n, 11)
    text, base_off, lw = rh.line_layout(seq, lb, gap)
    beg, end = rh.range_set(n, lb or n, lens_small=(0, 1, 65))
    assert (end - beg).max() == 200001
    want, ms = _device_equals_host(ctx, rh.blocks_at(text, 65280), rh.Ranges(base_off, lb or n, lw, beg, end), "long lb %s" % lb)
    assert want.tobytes() == rh.truth(seq, beg, end).tobytes() and ms[0] > 0 and ms[1] > 0


@pytest.mark.gpu
def test_gpu_gather_block_layouts_and_offsets_beyond_4g(ctx):
    seq = rh.bases(400_000, 21)
    text, base_off, lw = rh.line_layout(seq, 60, 1)
    blocks = rh.blocks_at(text, 65280)
    src = lambda i: base_off + (i // 60) * 61 + i % 60                         # noqa: E731
    blk = lambda i: src(i) // 65280                                              # noqa: E731
    # non-adjacent blocks, an empty one among them
    some = [blocks[0], (blocks[2][0], b""), blocks[2], blocks[3], (blocks[5][0], b""), blocks[5]]
    b0, b2, b5 = 100, 140_000, 330_000
    assert blk(b0) == 0 and blk(b2) == 2 and blk(b2 + 100_000) == 3 and blk(b5) == 5 and blk(b5 + 30_000) == 5
    R = rh.Ranges(base_off, 60, lw, [b5, b0, b2, b2, b2 + 50], [b5 + 30_000, b0 + 1, b2 + 100_000, b2, b2 + 99])
    want, _ = _device_equals_host(ctx, some, R, "non-adjacent")
    assert want.tobytes() == rh.truth(seq, R.beg, R.end).tobytes()
    # 1 range in 1 block; 3000 ranges in one block, unsorted, with duplicates and overlaps
    _device_equals_host(ctx, [blocks[1]], rh.Ranges(base_off, 60, lw, [70_000], [70_001]), "1 in 1")
    rng = np.random.default_rng(4)
    lo, hi = 66_000, 126_000
    assert blk(lo) == 1 and blk(hi) == 1
    beg = rng.integers(lo, hi - 300, 3000)
    beg[1000:2000] = beg[:1000]
    end = beg + rng.integers(0, 300, 3000)
    want, _ = _device_equals_host(ctx, [blocks[1]], rh.Ranges(base_off, 60, lw, beg, end), "3000 in 1")
    assert want.tobytes() == rh.truth(seq, beg, end).tobytes()
    # the same contig 2^32 - 130000 bytes further into its file: one range straddles 2^32, and so does one block
    far = (1 << 32) - 130_000
    far_blocks = [(u + far, d) for u, d in blocks]
    assert any(u < 1 << 32 < u + len(d) for u, d in far_blocks)
    i32 = next(i for i in range(200_000) if src(i) + far >= 1 << 32)
    R = rh.Ranges(base_off + far, 60, lw, [i32 - 5000, i32, 0, i32 - 1], [i32 + 5000, i32 + 70_000, 10, i32 + 1])
    want, _ = _device_equals_host(ctx, far_blocks[:4], R, "beyond 2^32")
    assert want.tobytes() == rh.truth(seq, R.beg, R.end).tobytes()


@pytest.mark.gpu
def test_gpu_gather_capacity_and_refusals(ctx):
    seq = rh.bases(9000, 3)
    text, base_off, lw = rh.line_layout(seq, 60, 1)
    blocks = rh.blocks_at(text, 2000)
    B, R = rh.Blocks(blocks), rh.Ranges(base_off, 60, lw, [0, 100, 5000], [4097, 100, 9000])
    total = 4097 + 4000
    rc, got, out_off, need, text_, guard, status, _ = rh.gather_device(ctx, B, R, cap=total - 1, guard=64)
    assert rc == _abi.OK and need == total and len(got) == 0 and (guard == 0xA5).all() and (status == 0x5A).all() and out_off.tolist() == [0, 4097, 4097, total]
    rc, got, _, need, _, guard, status, _ = rh.gather_device(ctx, B, R, cap=total, guard=64)
    assert rc == _abi.OK and need == total and got.tobytes() == rh.truth(seq, R.beg, R.end).tobytes() and (guard == 0xA5).all() and not status.any()
    rc, got, _, need, _, guard, status, _ = rh.gather_device(ctx, B, R, cap=total + 100, guard=64)        # room to spare: nothing behind the need is written
    assert rc == _abi.OK and need == total and (guard == 0xA5).all()
    for name, (blocks2, R2, why) in _refusals().items():
        rc, got, out_off, need, text_, guard, status, _ = rh.gather_device(ctx, rh.Blocks(blocks2), R2, cap=64, guard=64)
        assert rc == _abi.E_INVALID and why in text_ and text_.startswith("csv_ref_gather: "), (name, text_)
        assert (out_off == -7).all() and need == -7 and (guard == 0xA5).all() and (status == 0x5A).all(), name
    rc, _, out_off, need, text_, guard, status, _ = rh.gather_device(ctx, B, R, cap=total, guard=64, flags=1)
    assert rc == _abi.E_INVALID and "flags must be 0" in text_ and need == -7 and (guard == 0xA5).all() and (status == 0x5A).all()
    L = _lib.lib()
    z = np.zeros(4, np.int64)
    assert L.csv_ref_gather(None, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, z.ctypes.data, C.byref(C.c_int64()), None, 0, None) == _abi.E_INVALID
    for bad in (dict(n_blocks=-1), dict(n_ranges=-1), dict(out_off=None), dict(need=None), dict(cap=-1)):
        k = dict(n_blocks=0, n_ranges=0, out_off=z.ctypes.data, need=C.byref(C.c_int64()), cap=0)
        k.update(bad)
        rc = L.csv_ref_gather(ctx._h, None, 0, k["n_blocks"], None, None, None, None, None, k["n_ranges"], None, None, None, None, None, None, k["cap"], k["out_off"], k["need"], None, 0, None)
        assert rc == _abi.E_INVALID, bad
    need = C.c_int64(-7)
    assert L.csv_ref_gather(ctx._h, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, None, None, 0, z.ctypes.data, C.byref(need), None, 0, None) == _abi.OK
    assert need.value == 0
    # a payload outside comp
    B2 = rh.Blocks(blocks)
    B2.in_len = B2.in_len.copy(); B2.in_len[-1] += 1
    rc, _, _, need, text_, guard, status, _ = rh.gather_device(ctx, B2, R, guard=64)
    assert rc == _abi.E_INVALID and "the payload of block 4 lies outside comp" in text_ and (status == 0x5A).all()


@pytest.mark.gpu
def test_gpu_gather_with_a_damaged_block(ctx, tmp_path):
    seq = rh.bases(9000, 8)
    text, base_off, lw = rh.line_layout(seq, 60, 1)
    blocks = rh.blocks_at(text, 2000)
    R = rh.Ranges(base_off, 60, lw, [0, 3000, 8000], [2500, 7000, 9000])
    for kind, bit in (("crc", bam.INFLATE_STATUS["crc"]), ("truncate", None)):
        B = rh.Blocks(blocks, damage={2: kind})
        rc, got, out_off, need, _, guard, status, _ = rh.gather_device(ctx, B, R, cap=7600, guard=64)      # (100 bytes more than the need)
        assert rc == _abi.OK and need == 7500 and (guard == 0xA5).all(), kind
        assert status[2] != 0 and not status[[0, 1, 3, 4]].any() and (bit is None or status[2] == bit), (kind, status)
        assert got[:2500].tobytes() == seq[:2500] and got[-1000:].tobytes() == seq[8000:]         # ranges that read no damaged block are whole
    # through the reference: a flipped CRC is the host's to judge - it refuses the block too, with its own text; so does a cut payload
    ftext = rh.contig_text(b"c", seq, 60)
    pieces = rh.cut_text(ftext, 2000)
    for kind, why in (("crc", "fails its CRC32 or ISIZE"), ("truncate", "does not inflate|fails its CRC32")):
        image = bytearray(rh.bgzf_image(pieces))
        sizes = [len(bam_writer.bgzf_block(p, level=1)) for p in pieces]
        o2 = sum(sizes[:2])
        if kind == "crc":
            image[o2 + sizes[2] - 8] ^= 1
        else:                                                                 # the payload's second half becomes zeros: the block keeps its size
            image[o2 + 18 + (sizes[2] - 26) // 2:o2 + sizes[2] - 8] = bytes(sizes[2] - 26 - (sizes[2] - 26) // 2)
        gz = str(tmp_path / (kind + ".fa.gz"))
        with open(gz, "wb") as f:
            f.write(bytes(image))
        with open(gz + ".fai", "w") as f:
            f.write("c\t9000\t%d\t60\t61\n" % (len(ftext) - len(rh.contig_text(b"c", seq, 60)) + 11))
        ref = fasta.BgzfReference(gz)
        assert ref.offset[0] == 11
        host_err = dev_err = None
        try:
            ref.gather([0, 0], [0, 3000], [100, 7000], route="host")
        except fasta.BgzfReferenceError as e:
            host_err = str(e)
        try:
            ref.gather([0, 0], [0, 3000], [100, 7000], ctx=ctx, route="device")
        except fasta.BgzfReferenceError as e:
            dev_err = str(e)
        assert host_err is not None and re.search(why, host_err) and dev_err == host_err, (kind, host_err, dev_err)
        assert ref.stats["windows_host_after_device"] == 1
        blob, _ = ref.gather([0], [0], [1500], ctx=ctx, route="device")        # the undamaged part still answers, on the device
        assert blob.tobytes() == seq[:1500] and ref.stats["windows_device"] == 1


@pytest.mark.gpu
def test_gpu_gather_leaves_the_decode_columns_and_a_kept_rebuild_alone(ctx, tmp_path):
    import test_bam_reader as tbr
    import test_call_bam as tcb
    path = str(tmp_path / "edge.bam")
    tbr.write_edge(path)
    with bam.BamFile(path) as bf:
        (ch,) = list(bf.chunks("7"))
    use = np.ones(ch.n, np.uint8)
    keys = ("ins_read", "ins_pos", "ins_len", "ins_piece0", "ins_npiece", "piece_qoff", "piece_len", "del_read", "del_pos", "del_len")
    name, blocks, R, seq = _core_cases()[6]

    def gather():
        want, _ = _device_equals_host(ctx, blocks, R, name)
        assert len(want) > 50_000
    cols = bam.decode(ctx, ch)
    want = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
    cols = bam.decode(ctx, ch)
    gather()
    got = extract.cigar_signatures(ctx, None, None, None, use, min_siglength=5, from_bam=cols)
    assert want["n_sig_ins"] > 100
    for k in keys:
        assert np.array_equal(got[k], want[k]), k
    seqs, rb = tcb.alt_pool(ctx)
    src = rb["src_row"]
    ins_rows = np.flatnonzero(src < len(tcb.ALT_LENS))
    clip = np.asarray([len(seqs[int(src[r])]) for r in ins_rows], np.int64)
    want = rebuild.alt_gather_host(seqs, src, ins_rows, clip)
    gather()
    got = rebuild.alt_gather(ctx, ins_rows, clip)
    assert got[0] == want[0] and got[1].tolist() == want[1].tolist() and len(want[0]) > 1000
    rebuild.pool_reset(ctx); rebuild.name_pool_reset(ctx)


# ------------------------------------------------------------------------------------------------ GPU 2: end to end
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_ref")
    path = str(d / "planted.bam")
    ref = call_helpers.write_planted_bam(path)
    text = b"".join(rh.contig_text(c.encode(), s.encode(), 60, description=b"") for c, s in ref.items())
    plain, gz, image = rh.write_pair(d, text, 65280)
    return path, plain, gz, image


def _masked(data):
    return re.sub(rb"(?m)^##(fileDate|CommandLine)=.*$", rb"##\1=", data)


@pytest.mark.gpu
def test_gpu_call_bam_and_the_command_line_with_a_bgzipped_reference(ctx, planted, tmp_path):
    path, plain, gz, image = planted
    cp = call.CallParams(Params(min_support=1, genotype=True))
    kw = dict(ctx=ctx, as_bytes=True, report_readid=True, tra_gt="alignments")
    want, sv_want = call.call_bam(path, fasta.Reference(plain), cp, **kw)
    assert want.count(b"\n") >= 5 and b"SVTYPE=DEL" in want and b"SVTYPE=INS" in want
    for route in ("host", "device", None):
        ref = fasta.open_reference(gz)
        got, sv = call.call_bam(path, ref, cp, ref_route=route, **kw)
        assert got == want and sv.tolist() == sv_want.tolist(), route
        assert (ref.stats["windows_device"] > 0) == (route == "device") and ref.stats["windows_host_after_device"] == 0
    assert not os.path.exists(gz + ".fai") and not os.path.exists(gz + ".gzi")
    # the command line: ref.fa.gz for ref.fa, with neither index beside it, then with both
    wd = str(tmp_path / "work")
    os.mkdir(wd)
    outs, listing = {}, sorted(os.listdir(os.path.dirname(gz)))
    for name, ref_path, more in (("plain", plain, []), ("gz", gz, []), ("gz_device", gz, ["--ref_route", "device"])):
        out = str(tmp_path / (name + ".vcf"))
        assert cli.main([path, ref_path, out, wd, "-s", "1", "--genotype", "--report_readid"] + more) == 0
        with open(out, "rb") as f:
            outs[name] = _masked(f.read())
    assert outs["gz"] == outs["plain"] == outs["gz_device"] and outs["plain"].endswith(want)
    assert sorted(os.listdir(os.path.dirname(gz))) == listing                  # nothing was written next to the input
    assert fasta.main([gz, "--faidx", "--write"]) == 0
    with open(gz + ".fai") as f:
        fai = f.read()
    twin = fasta.Reference(plain)
    assert fai == "".join("%s\t%d\t%d\t%d\t%d\n" % (n, twin.length[i], twin.offset[i], twin.line_bases[i], twin.line_width[i]) for i, n in enumerate(twin.names))
    with open(gz + ".gzi", "rb") as f:
        assert f.read() == gzi_writer.gzi_bytes(image)
    out = str(tmp_path / "indexed.vcf")
    assert cli.main([path, gz, out, wd, "-s", "1", "--genotype", "--report_readid", "--ref_route", "device"]) == 0
    with open(out, "rb") as f:
        assert _masked(f.read()) == outs["plain"]
    tool = {}
    for name, ref_path, more in (("plain", plain, []), ("gz", gz, ["--ref_route", "device"])):
        out = str(tmp_path / ("tool_%s.vcf" % name))
        assert call.main([path, ref_path, "-o", out, "--preset", "ont", "--min_support", "1", "--genotype", "--report_readid"] + more) == 0
        with open(out, "rb") as f:
            tool[name] = f.read()
    assert tool["gz"] == tool["plain"] and tool["plain"].count(b"\n") >= 5
    os.remove(gz + ".fai"); os.remove(gz + ".gzi")


# ------------------------------------------------------------------------------------------------ the .fai from event rows
HDR = 1 << 62


def _events_host(h, window, base, row_cap=1 << 12, hdr_cap=1 << 12):
    """csv_fai_events_host on the window behind stream h -> (rows int64[n, 3] or None when they exceed row_cap, n_rows, tail, header texts)"""
    L = _lib.lib()
    carry, tail = np.zeros(3, np.int64), np.zeros(3, np.int64)
    assert L.csv_fasta_index_stream_carry(h, carry.ctypes.data) == _abi.OK
    rows, hdr = np.zeros((row_cap, 3), np.int64), np.zeros(hdr_cap, np.uint8)
    n_rows, hb = C.c_int64(-7), C.c_int64(-7)
    b = np.frombuffer(window, np.uint8) if window else np.zeros(0, np.uint8)
    rc = L.csv_fai_events_host(rh._ptr(b), len(b), base, carry.ctypes.data, rh._ptr(rows), row_cap, C.byref(n_rows), tail.ctypes.data, rh._ptr(hdr), hdr_cap, C.byref(hb))
    assert rc == _abi.OK and n_rows.value >= 0
    if n_rows.value > row_cap or hb.value > hdr_cap:
        return None, n_rows.value, tail, None
    return rows[:n_rows.value], n_rows.value, tail, hdr[:hb.value]


def _index_events(windows, as_bytes=()):
    """the index of the windows fed as event rows (the windows whose ordinal is in as_bytes: as bytes) -> as _index_stream, and every window's rows"""
    L = _lib.lib()
    h = L.csv_fasta_index_stream_open()
    all_rows, base = [], 0
    try:
        for k, w in enumerate(windows):
            b = np.frombuffer(w, np.uint8) if w else np.zeros(0, np.uint8)
            if k in as_bytes:
                L.csv_fasta_index_stream_feed(h, rh._ptr(b), len(b))
            else:
                rows, n, tail, hdr = _events_host(h, w, base)
                all_rows.append(rows.copy())
                L.csv_fasta_index_stream_rows(h, rh._ptr(rows), n, rh._ptr(hdr), len(hdr), len(w), tail.ctypes.data)
            base += len(w)
        cap = 16
        a = [np.zeros(cap, dt) for dt in (np.int64, np.int32, np.int64, np.int64, np.int32, np.int32)]
        names, nb = np.zeros(256, np.uint8), C.c_int64(0)
        n = L.csv_fasta_index_stream_finish(h, cap, names.ctypes.data, len(names), C.byref(nb), *[x.ctypes.data for x in a])
        if n < 0:
            return int(n), all_rows
        return [(names[int(a[0][i]):int(a[0][i]) + int(a[1][i])].tobytes(), int(a[2][i]), int(a[3][i]), int(a[4][i]), int(a[5][i])) for i in range(n)], all_rows
    finally:
        L.csv_fasta_index_stream_close(h)


def _cuts_of(text):
    yield [text]
    yield [text[i:i + 1] for i in range(len(text))]
    for cut in range(len(text) + 1):
        yield [text[:cut], text[cut:]]
        yield [text[:cut], b"", text[cut:cut + 2], text[cut + 2:]]


def test_the_event_row_form_equals_the_whole_index_at_every_cut():
    for text in STREAM_TEXTS:
        want = _index_whole(text)
        for windows in _cuts_of(text):
            assert _index_events(windows)[0] == want, (text, windows)
            assert _index_events(windows, as_bytes=(0,))[0] == want, (text, windows)          # bytes, then rows
            assert _index_events(windows, as_bytes=(1, 3))[0] == want, (text, windows)        # rows, bytes, rows, bytes
    for nl in (b"\n", b"\r\n"):
        text, _ = rh.crafted_fasta(nl, big=False)
        want = _index_whole(text)
        for step in (1, 7, 61, 64, 1000):
            got, rows = _index_events(rh.cut_text(text, step))
            assert got == want
        # the rows are few: a window's first line, the headers, the lines behind them, and the lines that differ from the one before
        got, rows = _index_events([text])
        assert len(rows[0]) <= 4 * len(want) and text.count(b"\n") > 20 * len(want)
        assert sum(1 for r in rows[0] if r[2] & HDR) == len(want)


def test_the_rows_assembler_refuses_rows_that_do_not_describe_the_window():
    L = _lib.lib()
    text = b">a\nACGT\nACGT\nAC\n"
    for spoil in ("start", "beyond", "gap", "tail", "hdr"):
        h = L.csv_fasta_index_stream_open()
        rows, n, tail, hdr = _events_host(h, text, 0)
        rows = rows.copy()
        assert rows.tolist() == [[0, 2, 2 | HDR], [3, 4, 4], [13, 2, 2]] and tail.tolist()[0] == len(text)
        if spoil == "start":
            rows[0, 0] = 1
        elif spoil == "beyond":
            rows[2, 1] = 40
        elif spoil == "gap":
            rows[2, 0] = 12
        elif spoil == "tail":
            tail[0] = len(text) + 1
        else:
            hdr = hdr[:1]
        assert L.csv_fasta_index_stream_rows(h, rows.ctypes.data, n, rh._ptr(hdr), len(hdr), len(text), tail.ctypes.data) == _abi.E_INVALID, spoil
        L.csv_fasta_index_stream_close(h)
    assert L.csv_fasta_index_stream_rows(None, None, 0, None, 0, 0, None) == _abi.E_INVALID and L.csv_fasta_index_stream_carry(None, None) == _abi.E_INVALID
    assert L.csv_fai_events_host(None, 0, 0, None, None, 0, None, None, None, 0, None) == _abi.E_INVALID


def _rows_per_window(gz, window_blocks=fasta.WINDOW_BLOCKS):
    """the host form's rows of every window fasta.BgzfReference cuts the file into (the index files beside it are not needed)"""
    none = os.path.join(os.path.dirname(gz), ".no-such-index")
    ref = fasta.BgzfReference(gz, fai=none, gzi=none, window_blocks=window_blocks)
    L = _lib.lib()
    h = L.csv_fasta_index_stream_open()
    counts = []
    try:
        for k0 in range(0, ref.n_blocks, ref.window_blocks):
            ks = np.arange(k0, min(k0 + ref.window_blocks, ref.n_blocks))
            data = ref._inflate_host(ks, *ref._payloads(ks)).tobytes()
            counts.append(_events_host(h, data, int(ref.uoff[k0]), row_cap=0, hdr_cap=0)[1])
            b = np.frombuffer(data, np.uint8)
            L.csv_fasta_index_stream_feed(h, rh._ptr(b), len(b))
    finally:
        L.csv_fasta_index_stream_close(h)
        ref.close()
    return counts


def _one_line_contigs(n=400):
    """every line differs from the one before: a row per line"""
    return b"".join(b">c%d\n" % k + rh.bases(50 + k, k) + b"\n" for k in range(n))


def _every_line_differs(n_lines=300):
    seq = rh.bases(n_lines * (n_lines + 1) // 2 + n_lines, 17)
    out, o = [b">odd\n"], 0
    for k in range(n_lines, 0, -1):                                          # (every line shorter than the one before: not indexable, but rows all the same)
        out.append(seq[o:o + k + 1] + b"\n")
        o += k + 1
    return b"".join(out)


def test_no_test_input_overflows_the_row_buffer_and_a_file_of_unequal_lines_does(tmp_path):
    """the count of overflow windows is 0 on every input of these tests: the host form's rows per window against the row buffer"""
    for j, (nl, big, cut) in enumerate([(b"\n", True, 65280), (b"\r\n", True, 65280), (b"\n", False, 61), (b"\n", False, 777), (b"\r\n", False, 1)]):
        text, _ = rh.crafted_fasta(nl, big=big)
        _, gz, _ = rh.write_pair(tmp_path, text, cut, name="r%d" % j)
        for wb in (fasta.WINDOW_BLOCKS, 3):
            counts = _rows_per_window(gz, wb)
            assert max(counts) <= 64 < fasta.FAI_ROW_CAP, (j, wb, max(counts))
    ref = call_helpers.write_planted_bam(str(tmp_path / "planted.bam"))          # the end-to-end test's reference
    text = b"".join(rh.contig_text(c.encode(), s.encode(), 60, description=b"") for c, s in ref.items())
    _, gz, _ = rh.write_pair(tmp_path, text, 65280, name="planted")
    assert max(_rows_per_window(gz)) <= 64
    _, gz, _ = rh.write_pair(tmp_path, _one_line_contigs(), 3000, name="odd")
    assert max(_rows_per_window(gz)) == 800 and max(_rows_per_window(gz, 4)) > 100 and fasta.FAI_ROW_CAP == 1 << 16


def test_the_event_core_under_the_sanitizers_gives_the_librarys_rows_and_index(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed (the library's own build needs it too)"
    exe = str(tmp_path / "ref_core_main")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "ref_core_main.cpp")], check=True, capture_output=True, text=True)
    sets = []
    for text in STREAM_TEXTS:
        sets += [[text], [text[i:i + 1] for i in range(len(text))], [text[:len(text) // 2], b"", text[len(text) // 2:]], rh.cut_text(text, 3)]
    for nl in (b"\n", b"\r\n"):
        text, _ = rh.crafted_fasta(nl, big=False)
        sets += [rh.cut_text(text, step) for step in (7, 61, 64, 1000)] + [[text]]
    sets.append(rh.cut_text(_every_line_differs(40), 50))
    for windows in sets:
        path = str(tmp_path / "windows.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(windows)) + b"".join(struct.pack("<I", len(w)) + w for w in windows))
        p = subprocess.run([exe, "events", path], capture_output=True)
        assert p.returncode == 0, (windows[:3], p.stderr[-3000:])
        want, rows = _index_events(windows)
        lines = p.stdout.split(b"\n")
        got_rows, at = [], 0
        for k in range(len(windows)):
            assert lines[at].startswith(b"window %d rows " % k)
            n = int(lines[at].split()[-1])
            got_rows.append([[int(x) for x in ln.split()] for ln in lines[at + 1:at + 1 + n]])
            at += 1 + n
        assert got_rows == [r.tolist() for r in rows]
        i_rows, i_bytes = lines.index(b"rows", at), lines.index(b"bytes", at)
        text_of = lambda a, b: lines[a + 1:b]                                                # noqa: E731
        mine = [b"refused"] if want == -_abi.E_INVALID else [b"%s %d %d %d %d" % e for e in want]
        assert text_of(i_rows, i_bytes) == mine and [ln for ln in lines[i_bytes + 1:] if ln] == mine, windows[:3]


# ---- GPU: k_fai_events
def _events_device(ctx, h, pieces, base, row_cap=1 << 12, hdr_cap=1 << 12):
    """csv_fai_events on the window whose blocks hold `pieces`, behind stream h -> as _events_host, and the status bytes"""
    L = _lib.lib()
    B = rh.Blocks([(0, p) for p in pieces])
    carry, tail = np.zeros(3, np.int64), np.zeros(3, np.int64)
    assert L.csv_fasta_index_stream_carry(h, carry.ctypes.data) == _abi.OK
    rows, hdr = np.full((row_cap + 2, 3), -7, np.int64), np.full(hdr_cap + 64, 0xA5, np.uint8)
    n_rows, hb, status = C.c_int64(-7), C.c_int64(-7), np.full(len(pieces), 0x5A, np.uint8)
    ctx._check(L.csv_fai_events(ctx._h, rh._ptr(B.comp), len(B.comp), len(pieces), rh._ptr(B.in_off), rh._ptr(B.in_len), rh._ptr(B.isize), rh._ptr(B.crc), base, carry.ctypes.data,
                                rows[1:].ctypes.data if row_cap else None, row_cap, C.byref(n_rows), tail.ctypes.data, hdr[32:].ctypes.data if hdr_cap else None, hdr_cap, C.byref(hb),
                                rh._ptr(status), None))
    n = n_rows.value
    fits = 0 <= n <= row_cap and hb.value <= hdr_cap
    # nothing outside rows[0, n) and hdr[0, hdr_bytes) is written
    assert (rows[0] == -7).all() and (rows[1 + (n if fits else 0):] == -7).all() and (hdr[:32] == 0xA5).all() and (hdr[32 + (hb.value if fits else 0):] == 0xA5).all()
    if not fits:
        return None, n, tail, None, status
    return rows[1:1 + n].copy(), n, tail, hdr[32:32 + hb.value].copy(), status


def _blocks_of(window, cut):
    return rh.cut_text(window, cut) if window else [b""]


@pytest.mark.gpu
def test_gpu_fai_events_rows_equal_the_host_forms_on_crafted_windows(ctx):
    L = _lib.lib()

    def run(windows, cut, want):
        h, g = L.csv_fasta_index_stream_open(), L.csv_fasta_index_stream_open()
        base = 0
        for w in windows:
            rows_h, n_h, tail_h, hdr_h = _events_host(h, w, base, row_cap=1 << 16, hdr_cap=1 << 16)
            rows_d, n_d, tail_d, hdr_d, status = _events_device(ctx, g, _blocks_of(w, cut), base, row_cap=1 << 16, hdr_cap=1 << 16)
            assert not status.any() and n_d == n_h and tail_d.tolist() == tail_h.tolist(), (windows[:2], cut, n_d, n_h)
            assert rows_d.tolist() == rows_h.tolist() and hdr_d.tobytes() == hdr_h.tobytes(), (windows[:2], cut)
            for s, rows, n, tail, hdr in ((h, rows_h, n_h, tail_h, hdr_h), (g, rows_d, n_d, tail_d, hdr_d)):
                L.csv_fasta_index_stream_rows(s, rh._ptr(rows), n, rh._ptr(hdr), len(hdr), len(w), tail.ctypes.data)
            base += len(w)
        for s in (h, g):
            cap = 16
            a = [np.zeros(cap, dt) for dt in (np.int64, np.int32, np.int64, np.int64, np.int32, np.int32)]
            names, nb = np.zeros(256, np.uint8), C.c_int64(0)
            n = L.csv_fasta_index_stream_finish(s, cap, names.ctypes.data, len(names), C.byref(nb), *[x.ctypes.data for x in a])
            got = int(n) if n < 0 else [(names[int(a[0][i]):int(a[0][i]) + int(a[1][i])].tobytes(), int(a[2][i]), int(a[3][i]), int(a[4][i]), int(a[5][i])) for i in range(n)]
            assert got == want, windows[:2]
            L.csv_fasta_index_stream_close(s)

    # the crafted texts, cut into two windows at every position (the cut between a base and its line break, between \r and \n, right
    # behind '>' are among them), each window one block
    for text in STREAM_TEXTS:
        want = _index_whole(text)
        for cut in range(len(text) + 1):
            run([text[:cut], text[cut:]], 65280, want)
    # the crafted FASTA: every line length around the wavefront, the 64-byte step and the tile; windows cut at the block cuts of the
    # fetch test; the big contigs cross the tile of 32768 bytes and the wavefronts' quarters of it
    for nl in (b"\n", b"\r\n"):
        text, _ = rh.crafted_fasta(nl, big=True)
        want = _index_whole(text)
        assert len(text) > 4 * 32768                                             # (five tiles)
        for step, cut in ((len(text), 65280), (100_000, 65280), (32768, 61), (8192 + 1, 4000), (65280, 62)):
            run(rh.cut_text(text, step), cut, want)
    # no line break at all in a window, and a window of empty blocks
    run([b">a\n" + b"A" * 70000, b"C" * 70000, b"", b"G" * 10 + b"\n"], 65280, [(b"a", 140010, 3, 140010, 140011)])


@pytest.mark.gpu
def test_gpu_fai_through_the_device_route_equals_the_plain_twins(ctx, tmp_path):
    for j, (nl, cut, wb) in enumerate([(b"\n", 65280, fasta.WINDOW_BLOCKS), (b"\r\n", 777, 5), (b"\n", 61, 64)]):
        text, seqs = rh.crafted_fasta(nl, big=j == 0)
        plain, gz, image = rh.write_pair(tmp_path, text, cut, name="d%d" % j)
        twin = fasta.Reference(plain)
        want = "".join("%s\t%d\t%d\t%d\t%d\n" % (n, twin.length[i], twin.offset[i], twin.line_bases[i], twin.line_width[i]) for i, n in enumerate(twin.names))
        ref = fasta.BgzfReference(gz, ctx=ctx, route="device", window_blocks=wb)
        assert ref.fai_built and ref.fai_text() == want
        st = ref.stats
        assert st["fai_windows_device"] == -(-ref.n_blocks // wb) and st["fai_windows_host"] == st["fai_windows_overflow"] == st["fai_windows_host_after_device"] == 0
        assert ref.fetch("lb61", 3, 200) == seqs["lb61"][3:200]
        host = fasta.BgzfReference(gz, route="host", window_blocks=wb)
        assert host.fai_text() == want and host.stats["fai_windows_host"] == st["fai_windows_device"] and host.stats["fai_windows_device"] == 0
        ref.close(); host.close(); twin.close()


@pytest.mark.gpu
def test_gpu_fai_window_that_overflows_the_row_buffer_is_the_host_forms(ctx, tmp_path, capsys):
    # lines of two lengths in turn: every line differs from the one before, the file is indexable only as one line per contig ...
    text = _one_line_contigs()
    plain, gz, image = rh.write_pair(tmp_path, text, 3000)
    twin = fasta.Reference(plain, write_fai=True)
    with open(plain + ".fai") as f:
        want = f.read()
    ref = fasta.BgzfReference(gz, ctx=ctx, route="device", window_blocks=4, fai_row_cap=100)
    assert ref.fai_text() == want
    st = ref.stats
    assert st["fai_windows_overflow"] > 0 and st["fai_windows_device"] > 0 and st["fai_windows_host"] == st["fai_windows_overflow"], st
    assert st["fai_windows_overflow"] == sum(1 for n in _rows_per_window(gz, 4) if n > 100)
    # ... header texts beyond their buffer are an overflow too
    ref2 = fasta.BgzfReference(gz, ctx=ctx, route="device", window_blocks=4, fai_hdr_cap=8)
    assert ref2.fai_text() == want and ref2.stats["fai_windows_overflow"] > 0
    # a damaged block: the device reports it, the host's verdict stands
    bad = bytearray(image)
    size0 = len(bam_writer.bgzf_block(rh.cut_text(text, 3000)[0], level=1))
    bad[size0 - 8] ^= 1
    gzb = str(tmp_path / "bad.fa.gz")
    with open(gzb, "wb") as f:
        f.write(bytes(bad))
    with pytest.raises(fasta.BgzfReferenceError, match="fails its CRC32 or ISIZE"):
        fasta.BgzfReference(gzb, ctx=ctx, route="device")
    # the command line on the device route
    assert fasta.main([gz, "--faidx", "--route", "device"]) == 0
    assert capsys.readouterr().out == want
    assert fasta.main([gz, "--faidx", "--route", "device", "--write"]) == 0
    with open(gz + ".fai") as f:
        assert f.read() == want
    with open(gz + ".gzi", "rb") as f:
        assert f.read() == gzi_writer.gzi_bytes(image)
    ref.close(); ref2.close(); twin.close()
