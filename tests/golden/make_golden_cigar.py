"""cigar_sigs.json.gz: the reference's parse_read (main script :606-681) driven with stub read objects (see
make_golden_main.py, which imports the main script and calls cigar_golden).
cigar_edges.json.gz: the same function on the crafted families and dense random reads of tests/cigar_helpers.py (cigar_edges)."""
import gzip
import json
import os

import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from cutesv_amd import synth                                  # noqa: E402  (pseudo_sequence: the fixtures store its key, not the bases)


class _Read:
    """what parse_read touches of a pysam.AlignedSegment"""

    def __init__(self, name, flag, mapq, start, cig, seq):
        self.query_name, self.flag, self.mapq, self.reference_start = name, flag, mapq, start
        self.cigartuples = cig
        self.cigar = cig
        self.query_sequence = seq
        self.query_length = len(seq)
        self.reference_end = start + sum(l for op, l in cig if op in (0, 2, 3, 7, 8))

    def get_tags(self):
        return []                                      # no SA tag: the split-read analysis is not on this path


def random_read(rng, name, kind, key):
    """kind: shapes the operation mix (ordinary / bursts of large indels / clips and exotic operations)"""
    ops = []
    n = int(rng.integers(1, 60 if kind != "long" else 400))
    if kind == "clips" and rng.random() < 0.7:
        ops.append((int(rng.choice([4, 5])), int(rng.integers(1, 300))))
    for _ in range(n):
        u = rng.random()
        if u < 0.45:
            ops.append((int(rng.choice([0, 7, 8])), int(rng.integers(1, 400))))
        elif u < 0.70:
            big = rng.random() < (0.5 if kind == "bursts" else 0.15)
            ops.append((1, int(rng.integers(10, 400)) if big else int(rng.integers(1, 10))))
        elif u < 0.95:
            big = rng.random() < (0.5 if kind == "bursts" else 0.15)
            ops.append((2, int(rng.integers(10, 400)) if big else int(rng.integers(1, 10))))
        elif kind == "clips":
            ops.append((int(rng.choice([3, 6])), int(rng.integers(1, 50))))       # N and P: the quirks of the shift counter
        else:
            ops.append((0, int(rng.integers(1, 30))))
    if kind == "clips" and rng.random() < 0.7:
        ops.append((int(rng.choice([4, 5])), int(rng.integers(1, 300))))
    # the query holds every operation that "consumes" the reference's shift counter so that slices never run off its end
    qlen = sum(l for op, l in ops if op != 2) + 8
    seq = synth.pseudo_sequence(qlen, key)
    return _Read(name, int(rng.choice([0, 16, 2048, 256])), int(rng.choice([0, 10, 20, 60])), int(rng.integers(0, 10_000_000)), ops, seq)


def cigar_golden(main):
    cases = []
    for name, seed, n, kind, params in (("ordinary", 11, 300, "plain", dict(min_siglength=10, mi=100, md=0)),
                                        ("bursts", 12, 300, "bursts", dict(min_siglength=10, mi=100, md=0)),
                                        ("bursts_md500", 13, 300, "bursts", dict(min_siglength=10, mi=1000, md=500)),
                                        ("clips_and_skips", 14, 300, "clips", dict(min_siglength=10, mi=100, md=100)),
                                        ("long_reads", 15, 40, "long", dict(min_siglength=30, mi=50, md=50)),
                                        ("siglength_1", 16, 100, "bursts", dict(min_siglength=1, mi=0, md=0))):
        rng = np.random.default_rng(seed)
        reads = [random_read(rng, "rd%05d" % i, kind, seed * 100000 + i) for i in range(n)]
        min_mapq, min_read_len = 20, 500
        cand = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
        for r in reads:
            main.parse_read(r, cand, "chr7", 30, min_mapq, 7, min_read_len, params["min_siglength"], params["md"], params["mi"], 100000)
        assert not cand["DUP"] and not cand["INV"] and not cand["TRA"]
        cases.append(dict(name=name, params=dict(params, min_mapq=min_mapq, min_read_len=min_read_len),
                          reads=[dict(name=r.query_name, flag=r.flag, mapq=r.mapq, start=r.reference_start, cigar=[list(x) for x in r.cigartuples],
                                      seq_len=len(r.query_sequence), seq_key=seed * 100000 + i) for i, r in enumerate(reads)],
                          INS=[list(x) for x in cand["INS"]], DEL=[list(x) for x in cand["DEL"]]))
    with gzip.open(os.path.join(HERE, "cigar_sigs.json.gz"), "wt") as f:
        json.dump(cases, f)
    print("cigar_sigs.json.gz: %d cases, %d INS + %d DEL signatures" % (len(cases), sum(len(c["INS"]) for c in cases), sum(len(c["DEL"]) for c in cases)))


# ------------------------------------------------------------------------------------------------ cigar_edges.json.gz
def _run(main, reads, params, min_mapq, min_read_len):
    """parse_read on every read -> per read {"INS": rows, "DEL": rows}"""
    out = []
    for r in reads:
        cand = {t: [] for t in ("DEL", "INS", "DUP", "INV", "TRA")}
        rd = _Read(r["name"], r["flag"], r["mapq"], r["start"], [tuple(x) for x in r["cigar"]], synth.pseudo_sequence(r["seq_len"], r["seq_key"]))
        main.parse_read(rd, cand, "chr7", 30, min_mapq, 7, min_read_len, params["min_siglength"], params["md"], params["mi"], 100000)
        assert not cand["DUP"] and not cand["INV"] and not cand["TRA"]
        out.append(dict(INS=[list(x) for x in cand["INS"]], DEL=[list(x) for x in cand["DEL"]]))
    return out


def cigar_edges(main):
    """crafted families (tests/cigar_helpers.py) and dense random reads through the reference's parse_read -> cigar_edges.json.gz"""
    import hashlib
    sys.path.insert(0, os.path.dirname(HERE))
    import cigar_helpers as ch
    cases = []
    for k, (set_name, params) in enumerate(ch.PARAM_SETS.items()):
        for name, reads, gates, expect in (("edges_" + set_name, ch.families(set_name, params, 7000000 + 10000 * k), dict(min_mapq=20, min_read_len=0), ch.expectations(params)),
                                           ("host_" + set_name, ch.host_family(set_name, params, 7500000 + 10000 * k), dict(ch.HOST_PARAMS), ch.HOST_EXPECTATIONS)):
            per_read = _run(main, reads, params, gates["min_mapq"], gates["min_read_len"])
            # self-check, on the reference alone and free of names and bases: every family is there and does what it is there to show
            ch.check_families(reads, [(o["INS"], o["DEL"]) for o in per_read], expect)
            # (this tests the table; it speaks for the reads because check_families has just required their families to be the table's keys)
            assert {ch.kind_of(f) for f in expect} == set(ch.FAMILY_KINDS if name.startswith("edges_") else ("host",)), "a family kind is missing for %s" % set_name
            cases.append(dict(name=name, params=dict(params, **gates), reads=reads, INS=[x for o in per_read for x in o["INS"]],
                              DEL=[x for o in per_read for x in o["DEL"]]))
    crafted_ins = [x for c in cases for x in c["INS"]]
    assert any(x[3] == "" for x in crafted_ins) and any(0 < len(x[3]) < x[1] for x in crafted_ins), "no INS slice is cut by the query's end"
    for k, params in enumerate(ch.DENSE_SETS):
        seed, n = 8100 + k, 3000
        reads = ch.dense_reads(seed, n)
        cnt = ch.counters(reads, params)
        assert all(v >= 100 for v in cnt.values()), "dense_%d: a decision occurs fewer than 100 times: %s" % (k, cnt)
        per_read = _run(main, reads, params, 20, 0)
        ins, dele = [x for o in per_read for x in o["INS"]], [x for o in per_read for x in o["DEL"]]
        dump = lambda rows: hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()      # noqa: E731
        cases.append(dict(name="dense_%d" % k, params=dict(params, min_mapq=20, min_read_len=0), dense=dict(seed=seed, n=n, checksum=ch.reads_checksum(reads)),
                          n_ins=len(ins), n_del=len(dele), sha_ins=dump(ins), sha_del=dump(dele), per_read=ch.per_read_digests(reads, ins, dele), counters=cnt))
        print("  dense_%d %s: %d INS + %d DEL rows; %s" % (k, params, len(ins), len(dele), cnt))
    path = os.path.join(HERE, "cigar_edges.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases).encode())
    assert os.path.getsize(path) < 400 * 1024
    print("cigar_edges.json.gz: %d cases, %d crafted reads, %d bytes" % (len(cases), sum(len(c.get("reads", ())) for c in cases), os.path.getsize(path)))
