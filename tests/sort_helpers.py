"""Shared by tests/test_bam_sort.py and scripts/sort_stage.py: the judge of the coordinate sort and the inputs.

The judge is an independent restatement: it parses the inflated stream of the INPUT with `struct`, orders the records with Python's
stable `sorted` on (refid as unsigned, pos, reverse-strand bit), rewrites the header text by its own reading of the header rule and
joins the bytes.  It shares no code with cutesv_amd; the output files are read back with `gzip` from the standard library."""
import gzip
import struct

import numpy as np

import bam_writer

BLOCK = 65280


def inflate_file(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def split_stream(stream):
    """the inflated stream of a BAM -> (header bytes, [record bytes, block_size word included])"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", stream, o)[0]
    head, recs = stream[:o], []
    while o < len(stream):
        bs = struct.unpack_from("<i", stream, o)[0]
        recs.append(stream[o : o + 4 + bs])
        o += 4 + bs
    assert o == len(stream)
    return head, recs


def key_of(rec):
    refid, pos = struct.unpack_from("<ii", rec, 4)
    flag = struct.unpack_from("<H", rec, 18)[0]
    return (refid & 0xFFFFFFFF, pos, (flag >> 4) & 1)


def judge_header(head):
    """the header rule, restated: @HD's SO: becomes coordinate (appended when absent), GO: and SS: leave, no @HD: one is put first"""
    l_text = struct.unpack_from("<i", head, 4)[0]
    text, rest = head[8 : 8 + l_text], head[8 + l_text :]
    lines = text.split(b"\n")
    k = next((i for i, ln in enumerate(lines) if ln == b"@HD" or ln.startswith(b"@HD\t")), None)
    if k is None:
        text = b"@HD\tVN:1.6\tSO:coordinate\n" + text
    else:
        fields, seen = [], False
        for f in lines[k].split(b"\t")[1:]:
            if f.startswith(b"SO:"):
                if not seen:
                    fields.append(b"SO:coordinate")
                seen = True
            elif not f.startswith((b"GO:", b"SS:")):
                fields.append(f)
        if not seen:
            fields.append(b"SO:coordinate")
        lines[k] = b"\t".join([b"@HD"] + fields)
        text = b"\n".join(lines)
    return b"BAM\1" + struct.pack("<i", len(text)) + text + rest


def judge(stream):
    """the inflated stream of the input -> (the stream the sorted file must inflate to, its header, the records in order, the permutation)"""
    head, recs = split_stream(stream)
    order = sorted(range(len(recs)), key=lambda i: key_of(recs[i]))
    new_head = judge_header(head)
    ordered = [recs[i] for i in order]
    return new_head + b"".join(ordered), new_head, ordered, order


def inversions(stream):
    _, recs = split_stream(stream)
    keys = [key_of(r) for r in recs]
    return sum(1 for a, b in zip(keys, keys[1:]) if b < a)


def tiny(name, refid, pos, flag=0, seq="", cigar=(), tags=()):
    """a shortest-form record: no CIGAR, no bases unless asked for - 37 bytes plus the name"""
    return dict(name=name, flag=flag, mapq=20, start=pos, cigar=list(cigar), seq=seq, tags=list(tags), refid=refid)


def random_tiny(n, seed, n_ref=2, max_pos=50000, unmapped=0.1, name="q%d"):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        if rng.random() < unmapped:
            recs.append(tiny(name % i, -1, -1, flag=4))
        else:
            recs.append(tiny(name % i, int(rng.integers(0, n_ref)), int(rng.integers(0, max_pos)), flag=16 if rng.random() < 0.5 else 0,
                             seq="ACGT"[: int(rng.integers(0, 5))]))
    return recs


def raw_record(r):
    """bam_writer.record_bytes for a record at any position up to 2^31 - 2: built at a small position, then pos is patched (the bin
    field keeps the small position's value: nothing here reads it)"""
    blob = bytearray(bam_writer.record_bytes(dict(r, start=min(r["start"], 1000)))[0])
    struct.pack_into("<i", blob, 8, r["start"])
    return bytes(blob)


def write_stream(path, stream, block_bytes=BLOCK):
    """a raw inflated stream as a BGZF file: for inputs patched after bam_writer built them"""
    with open(path, "wb") as f:
        for a in range(0, len(stream), block_bytes):
            f.write(bam_writer.bgzf_block(stream[a : a + block_bytes]))
        f.write(bam_writer.EOF_BLOCK)


def header_bytes(text, refs):
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, ln in refs:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return head


def blocks_of(blob):
    """the BGZF blocks of a file's bytes -> [(offset, size, isize)]"""
    out, o = [], 0
    while o < len(blob):
        assert blob[o : o + 4] == b"\x1f\x8b\x08\x04" and blob[o + 12 : o + 14] == b"BC", o
        size = struct.unpack_from("<H", blob, o + 16)[0] + 1
        out.append((o, size, struct.unpack_from("<I", blob, o + size - 4)[0]))
        o += size
    assert o == len(blob)
    return out


def keep_ties_permutation(recs, seed):
    """a shuffle of `recs` in which records of equal key keep their relative order: shuffle, then restore ascending original ordinals
    inside each equal-key group -> the permuted list"""
    rng = np.random.default_rng(seed)
    idx = [int(i) for i in rng.permutation(len(recs))]
    kf = lambda r: (r.get("refid", 0) & 0xFFFFFFFF, r["start"], (r["flag"] >> 4) & 1)       # noqa: E731
    slots = {}
    for at, i in enumerate(idx):
        slots.setdefault(kf(recs[i]), []).append(at)
    out = list(idx)
    for k, where in slots.items():
        members = sorted(idx[at] for at in where)
        for at, i in zip(where, members):
            out[at] = i
    return [recs[i] for i in out]
