"""Crafted call tables for the record core (cutesv_amd/csrc/vcf_core.h) and the raw faces of the three emitters that take
REF bases per call: csv_vcf_emit_ref (the yardstick), csv_vcf_emit_core_host (the core with one lane) and csv_vcf_emit_device (the kernels).

A Table is everything a csv_vcf_in is made of, as plain Python: chromosomes with their sequences, segments, calls, and per call the ALT and
RNAMES bytes.  `vin(table, **flags)` builds the struct (and keeps its arrays alive), `ref_of` the per-call REF blob from csv_vcf_ref_ranges,
`run(entry, ...)` calls an emitter behind a guard of 64 bytes."""
import ctypes as C

import numpy as np

from cutesv_amd import _abi
from cutesv_amd._lib import lib
from cutesv_amd.genotype import gl_fields, gl_index

DEL, INS, DUP, INV, TRA = _abi.DEL, _abi.INS, _abi.DUP, _abi.INV, _abi.TRA
GUARD = 64
P31 = (1 << 31) - 1
IUPAC = "RYSWKMBDHVNacgtryswkmbdhvnACGT"
FLAG_SETS = [dict(genotype=g, report_readid=r, ignore_sequence=i) for g in (False, True) for r in (False, True) for i in (False, True)]
SIZE_SETS = [dict(min_size=30, max_size=100000), dict(min_size=10, max_size=500), dict(min_size=30, max_size=-1)]


class Table:
    def __init__(self, chroms, seqs, strands=("++", "--")):
        self.chroms, self.seqs, self.strands = list(chroms), dict(seqs), tuple(strands)
        self.segs, self.calls = [], []

    def seg(self, svtype, chrom, genotype):
        self.segs.append((svtype, self.chroms.index(chrom), int(genotype)))
        return len(self.segs) - 1

    def call(self, seg, bp1, bp2, support=3, aux=0, cipos=0, cilen=0, dr=-1, gl=-1, alt=b"", rn=b""):
        self.calls.append(dict(seg=seg, bp1=bp1, bp2=bp2, support=support, aux=aux, cipos=cipos, cilen=cilen, dr=dr, gl=gl, alt=alt, rn=rn))

    @property
    def n(self):
        return len(self.calls)

    def column(self, key):
        return np.array([c[key] for c in self.calls], np.int64)


class Columns(Table):
    """a Table whose calls are numpy columns (no ALT, no RNAMES): for the tables of a million calls"""

    def __init__(self, chroms, seqs, **cols):
        Table.__init__(self, chroms, seqs)
        self.cols = {k: np.asarray(v, np.int64) for k, v in cols.items()}
        self.calls = _NoStrings(len(self.cols["bp1"]))

    def column(self, key):
        return self.cols[key] if key in self.cols else np.full(len(self.calls), dict(support=3, dr=-1, gl=-1).get(key, 0), np.int64)


class _NoStrings:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(())


def af_table(dv, dr):
    """one genotyped DUP call per (dv, dr): the smallest record that carries ;AF="""
    t = Columns(["c"], {"c": b"ACGT" * 8}, bp1=np.full(len(dv), 5), bp2=np.full(len(dv), 9), support=dv, dr=dr, gl=np.full(len(dv), gl_index(10, 10)))
    t.seg(DUP, "c", 1)
    return t


def sequence(n, seed):
    """n bases: ACGT at random, with every IUPAC code and lower case at the head, at the tail and every 97 bases"""
    rng = np.random.default_rng(seed)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    code = np.frombuffer(IUPAC.encode(), np.uint8)
    k = min(n, len(code))
    s[:k] = code[:k]
    s[n - k:] = code[:k][::-1]
    s[::97] = code[np.arange(len(s[::97])) % len(code)]
    return s.tobytes()


class Built:
    """a csv_vcf_in with everything it points to"""


def vin(t, min_size=30, max_size=100000, genotype=False, report_readid=False, ignore_sequence=False, gl_keys=None, with_strings=True):
    b = Built()
    n = t.n
    b.res = _abi.HostResult(0, max(1, n), 1, no_support=True)
    for name, key in (("call_seg", "seg"), ("call_aux", "aux"), ("bp1", "bp1"), ("bp2", "bp2"), ("support", "support"), ("cipos", "cipos"), ("cilen", "cilen"),
                      ("dr", "dr"), ("gl_idx", "gl"), ("dv", "support")):
        b.res.arrays[name][:n] = t.column(key)
    b.res.c.n_calls = n
    b.segs = np.zeros(max(1, len(t.segs)), _abi.SEGMENT_DTYPE)
    for k, (ty, ch, gt) in enumerate(t.segs):
        b.segs[k]["svtype"], b.segs[k]["chrom"], b.segs[k]["genotype"] = ty, ch, gt
    nch = len(t.chroms)
    b.names = (C.c_char_p * max(1, nch))(*[c.encode() for c in t.chroms])
    b.clen = np.array([len(t.seqs.get(c, b"")) for c in t.chroms] + [0], np.int64)
    order = sorted(range(nch), key=lambda i: t.chroms[i])
    b.rank = np.zeros(max(1, nch), np.int32)
    b.rank[order] = np.arange(nch, dtype=np.int32)
    b.alt_off, b.rn_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    if n and not isinstance(t.calls, _NoStrings):
        b.alt_off[1:] = np.cumsum([len(c["alt"]) for c in t.calls])
        b.rn_off[1:] = np.cumsum([len(c["rn"]) for c in t.calls])
    b.alt, b.rn = b"".join(c["alt"] for c in t.calls), b"".join(c["rn"] for c in t.calls)
    gl = t.column("gl")
    keys = np.unique(gl[gl >= 0]).tolist() if gl_keys is None else list(gl_keys)
    b.keys = np.array(keys + [0], np.int32)
    b.gl_strs = (C.c_char_p * max(1, len(keys)))(*["\t".join(gl_fields(int(k))).encode() for k in keys])
    b.strands = (C.c_char_p * len(t.strands))(*[s.encode() for s in t.strands])
    b.c = _abi.VcfIn(res=C.pointer(b.res.c), seg=b.segs.ctypes.data, n_seg=len(t.segs), n_chrom=nch, chrom_name=b.names, chrom_seq=None, chrom_len=b.clen.ctypes.data,
                     chrom_rank=b.rank.ctypes.data, chrom_line_bases=None, chrom_line_width=None,
                     ins_alt=b.alt if with_strings else None, ins_alt_off=b.alt_off.ctypes.data if with_strings else None,
                     rnames=b.rn if with_strings else None, rnames_off=b.rn_off.ctypes.data if with_strings else None,
                     strand_name=b.strands, gl_key=b.keys.ctypes.data, gl_str=b.gl_strs, n_gl=len(keys), min_size=min_size, max_size=max_size, genotype=int(genotype),
                     report_readid=int(report_readid), ignore_sequence=int(ignore_sequence))
    return b


def ref_of(t, b):
    """csv_vcf_ref_ranges and a gather from the table's sequences -> (rc, blob uint8, off int64[n + 1])"""
    n = t.n
    beg, end, chrom = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int32)
    rc = lib().csv_vcf_ref_ranges(C.byref(b.c), beg.ctypes.data, end.ctypes.data, chrom.ctypes.data)
    if rc:
        return rc, np.zeros(0, np.uint8), np.zeros(n + 1, np.int64)
    beg, end, chrom = beg[:n], end[:n], chrom[:n]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(end - beg, out=off[1:])
    if isinstance(t.calls, _NoStrings):                      # (one contig, one base per call)
        seq = np.frombuffer(t.seqs[t.chroms[0]], np.uint8)
        assert ((end - beg) == 1).all()
        return 0, seq[beg].copy(), off
    blob = b"".join(t.seqs[t.chroms[int(chrom[c])]][int(beg[c]):int(end[c])] for c in np.flatnonzero(end > beg).tolist())
    assert len(blob) == off[-1]
    return 0, np.frombuffer(blob, np.uint8).copy(), off


def dump(path, t, b, blob, off, svid):
    """the csv_vcf_in of `b` with its REF blob as the file tests/vcf_core_main.cpp reads"""
    import struct
    n, c = t.n, b.c
    names = [x.encode() for x in t.chroms]
    keys = b.keys[:c.n_gl]
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", n, len(t.segs), len(names), c.n_gl, len(t.strands), c.min_size, c.max_size, 0))
        f.write(struct.pack("<4i", c.genotype, c.report_readid, c.ignore_sequence, 0))
        for key in ("seg", "aux", "support", "cipos", "cilen", "dr", "gl"):
            f.write(t.column(key).astype(np.int32).tobytes())
        for key in ("bp1", "bp2"):
            f.write(t.column(key).astype(np.int64).tobytes())
        for field in ("svtype", "chrom", "genotype"):
            f.write(np.ascontiguousarray(b.segs[field][:len(t.segs)], np.int32).tobytes())
        f.write(b.clen[:len(names)].tobytes() + b.rank[:len(names)].tobytes())
        for x in names + [x.encode() for x in t.strands] + ["\t".join(gl_fields(int(k))).encode() for k in keys]:
            f.write(struct.pack("<i", len(x)) + x)
        f.write(np.ascontiguousarray(keys, np.int32).tobytes())
        for o, blob_ in ((b.alt_off, b.alt), (b.rn_off, b.rn), (off, blob.tobytes())):
            f.write(np.ascontiguousarray(o, np.int64).tobytes() + struct.pack("<q", len(blob_)) + blob_)
        f.write(np.ascontiguousarray(svid, np.int64).tobytes())


class Out:
    pass


def run(entry, b, blob, off, svid=None, cap=None, ctx=None, prefix=b"", flags=0, rows=True, pick=None, clip=None):
    """entry: "ref" (csv_vcf_emit_ref), "core" (csv_vcf_emit_core_host) or "device" (csv_vcf_emit_device on ctx) -> Out with rc, need, text (the
    bytes written when rc is 0), svid (after the call), guard_ok (the 64 bytes behind `cap` are untouched, and on a failure every byte in
    front of them as well), rows / names_chrom (device)"""
    L = lib()
    o = Out()
    o.svid = np.zeros(5, np.int64) if svid is None else np.array(svid, np.int64)
    n = int(b.res.c.n_calls)
    if cap is None:
        cap = 512 * max(n, 1) + len(blob) + len(b.alt) + len(b.rn) + len(prefix) + 4096
    buf = np.full(cap + GUARD, 0xA5, np.uint8)
    need = C.c_int64(-7)
    ptr = blob.ctypes.data if len(blob) else None
    if entry == "ref":
        o.rc = L.csv_vcf_emit_ref(C.byref(b.c), ptr, off.ctypes.data, C.cast(buf.ctypes.data, C.c_char_p), cap, C.byref(need), o.svid.ctypes.data)
    elif entry == "core":
        o.rc = L.csv_vcf_emit_core_host(C.byref(b.c), ptr, off.ctypes.data, buf.ctypes.data, cap, C.byref(need), o.svid.ctypes.data)
    else:
        o.rows_buf, o.name_chrom = np.full((max(n, 1), 4), -1, np.int64), np.full(max(1, b.c.n_chrom), -1, np.int32)
        n_rows, n_names, ms = C.c_int64(-1), C.c_int32(-1), C.c_double(0)
        pk = None if pick is None else np.ascontiguousarray(pick, np.int64)
        cl = None if clip is None else np.ascontiguousarray(clip, np.int64)
        o.rc = L.csv_vcf_emit_device(ctx._h, C.byref(b.c), ptr, off.ctypes.data, 0 if pk is None else len(pk), None if pk is None or not len(pk) else pk.ctypes.data,
                                     None if cl is None or not len(cl) else cl.ctypes.data, prefix if prefix else None, len(prefix), flags, buf.ctypes.data if cap else None, cap,
                                     C.byref(need), o.svid.ctypes.data, o.rows_buf.ctypes.data if rows else None, len(o.rows_buf) if rows else 0, C.byref(n_rows),
                                     o.name_chrom.ctypes.data, C.byref(n_names), C.byref(ms))
        o.n_rows, o.n_names, o.ms = n_rows.value, n_names.value, ms.value
        o.rows = o.rows_buf[:max(0, o.n_rows)]
        o.error = (L.csv_last_error(ctx._h) or b"").decode()
    o.need = need.value
    o.text = buf[:o.need].tobytes() if o.rc == 0 else b""
    wrote_to = o.need if o.rc == 0 else 0
    o.guard_ok = bool((buf[wrote_to:] == 0xA5).all())
    return o


# ------------------------------------------------------------------------------------------------ the crafted table
PAIRS = [(0, 10), (10, 10), (30, 2), (100, 1), (3, 1), (6, 2), (1, 31), (157, 3)]          # (DR, DV): 1/1, 0/1, 0/0 (IMPRECISE, q5), the two special keys, 1/32, 3/160


def _names(k, seed):
    return ",".join("read/%d_%d" % (seed, j) for j in range(k)).encode()


def crafted():
    """all five types, the four BND codes and both strands, mates on other contigs, positions at digit boundaries and at the contigs' ends,
    sizes at the filters' thresholds between kept ones, genotyped and not, gl_idx -1, on contigs named with 1 and with 40 bytes and one
    contig without calls between them in the emission order"""
    chroms = ["chrB", "A", "N0", "Z" * 40]
    lens = {"chrB": 3000, "A": 100000, "N0": 500, "Z" * 40: 5000}
    t = Table(chroms, {c: sequence(lens[c], 11 + i) for i, c in enumerate(chroms)})
    sizes = [30, 99, 100, 999, 1000, 9999, 10000, 100000, 100001, 29, 5, 500, 501, 10, 9]
    supports, cis = [1, 9, 10, 99, 100, 1000], [0, 9, 10, 99]
    k = 0
    for name in ("chrB", "A", "Z" * 40):
        S, ci = lens[name], chroms.index(name)
        pos = [0, 1, 9, 10, 99, 100, S - 2, S - 1]
        for gt in (0, 1):
            def extra():
                nonlocal k
                k += 1
                dr, dv = PAIRS[k % len(PAIRS)]
                lost = gt and k % 5 == 0                                          # count_coverage gave up: gl_idx -1, DR -1
                return dict(support=dv if gt else supports[k % 6], cipos=cis[k % 4], cilen=cis[(k // 4) % 4], dr=(-1 if lost else dr) if gt else -1,
                            gl=(-1 if lost else gl_index(dr, dv)) if gt else -1, rn=b"" if k % 7 == 0 else _names(1 + k % 4, k))
            sd, si, su, sv, sb = (t.seg(ty, name, gt) for ty in (DEL, INS, DUP, INV, TRA))
            for pi, p in enumerate(pos):
                for zi, z in enumerate(sizes):
                    t.call(sd, p, z, **extra())
                    t.call(si, p, z, alt=sequence(min(z, 300), z + p)[: (0 if (z + p) % 11 == 0 else min(z, 300))], **extra())
                    t.call(su, p, p + z, **extra())
                    t.call(sv, p, p - z if zi % 3 == 0 else p + z, aux=(pi + zi) % 2, **extra())
            mates = [c for c in range(len(chroms)) if c != ci]
            for p in pos + [S, S + 1, P31]:
                for code in range(4):
                    for m, bp2 in zip(mates, (0, 99999, P31)):
                        t.call(sb, p, bp2, aux=m * 8 + code, **extra())
    return t


def shaped(n_calls, lengths, seed=5):
    """n_calls calls on one contig of 6000 bases cycling through DEL (REF of the lengths), INS (ALT of the lengths), DUP, INV, BND, every one with
    RNAMES of the lengths: the shapes at which the plan grid, the scan tile and the lanes' loops turn over"""
    t = Table(["c", "m"], {"c": sequence(6000, seed), "m": sequence(50, seed + 1)})
    segs = [t.seg(ty, "c", 0) for ty in (DEL, INS, DUP, INV, TRA)]
    filler = sequence(max(lengths) + 1, seed + 2)
    for i in range(n_calls):
        z = lengths[i % len(lengths)]
        ty = i % 5
        p = 1 + (i * 37) % 900
        rn = filler[: lengths[(i // 5) % len(lengths)]].replace(b";", b"x")
        if ty == 0:
            t.call(segs[0], p, max(z - 1, 0), rn=rn)                            # REF = bases [p - 1, p + len): len + 1 of them
        elif ty == 1:
            t.call(segs[1], p, 40, alt=filler[:z], rn=rn)
        elif ty == 2:
            t.call(segs[2], p, p + 50, rn=rn)
        elif ty == 3:
            t.call(segs[3], p, p + 50, aux=i % 2, rn=rn)
        else:
            t.call(segs[4], p, 7, aux=8 + i % 4, rn=rn)
    return t
