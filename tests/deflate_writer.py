"""A bit writer for RFC 1951 and the corpus of DEFLATE streams the BGZF inflate tests run (tests/test_bgzf_inflate.py).

It shares no code with the decoder under test (cutesv_amd/csrc/inflate_core.h): streams are put together bit by bit from the
RFC's tables, so that the shapes zlib's compressor never emits exist - a length written as symbol 284 with extra 31, a code of
15 bits, a repeat that runs from the literal/length lengths into the distance lengths, a damaged header.  zlib's INFLATE is the
judge of the corpus itself: every valid entry must inflate to the intended bytes, every damaged one must fail (the self-check
in test_bgzf_inflate.py).

    corpus() -> [Entry]       name, payload (raw deflate), data (the bytes it stands for; None when damaged), isize, crc,
                              bit (0, or the one status bit csv_bgzf_inflate must report), stream (damaged: zlib itself
                              raises on the payload; else the damage is in ISIZE or the CRC)

On "HCLEN 4": a dynamic header with four code-length codes (16, 17, 18, 0) can only spell lengths of zero, and zlib refuses a
block without an end-of-block code - no valid block of that kind exists.  The corpus holds the damaged block with four, and
valid blocks with eight (HCLEN field 4) and with all nineteen.
"""
import random
import struct
import zlib
from collections import namedtuple

Entry = namedtuple("Entry", "name payload data isize crc bit stream")

# the status bits of csv_bgzf_inflate (include/cutesv_hip.h)
E_HEADER, E_LENGTHS, E_SYMBOL, E_DISTANCE, E_OUTPUT, E_SHORT, E_INPUT, E_CRC = 1, 2, 4, 8, 16, 32, 64, 128

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: (base, extra bits) of length symbols 257 .. 285 and of distance symbols 0 .. 29
LEN_TAB = [(3 + i, 0) for i in range(8)] + [(b, e) for e in range(1, 6) for b in [((4 + k) << e) + 3 for k in range(4)]] + [(258, 0)]
DIST_TAB = [(1 + i, 0) for i in range(4)] + [(((2 + k) << e) + 1, e) for e in range(1, 14) for k in range(2)]
assert len(LEN_TAB) == 29 and LEN_TAB[8] == (11, 1) and LEN_TAB[27] == (227, 5) and len(DIST_TAB) == 30 and DIST_TAB[29] == (24577, 13)


class Bits:
    """bits are packed starting at the least significant bit of a byte (RFC 1951 3.1.1)"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """a data element: least significant bit first"""
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """a Huffman code: most significant bit first"""
        self.put(int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    @property
    def bit_position(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)"""
    count = [0] * 16
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


FIXED_LL = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = canonical([5] * 32)
assert FIXED_LL[0] == (0x30, 8) and FIXED_LL[144] == (0x190, 9) and FIXED_LL[256] == (0, 7) and FIXED_LL[280] == (0xC0, 8)


def length_symbol(length, long_form=False):
    """-> (symbol, extra bits, extra value); long_form: 258 as symbol 284 with extra 31"""
    if length == 258 and not long_form:
        return 285, 0, 0
    s = max(i for i, (b, e) in enumerate(LEN_TAB[:28]) if b <= length)
    b, e = LEN_TAB[s]
    assert length - b < (1 << e) or e == 0 and length == b
    return 257 + s, e, length - b


def dist_symbol(dist):
    s = max(i for i, (b, e) in enumerate(DIST_TAB) if b <= dist)
    b, e = DIST_TAB[s]
    assert dist - b < (1 << e) or (e == 0 and dist == b)
    return s, e, dist - b


def put_symbols(w, ll, d, symbols):
    """symbols: ('lit', v) | ('match', length, dist[, long_form]) | ('ll', symbol) | ('d', symbol) | ('bits', value, n) | ('eob',)"""
    for t in symbols:
        if t[0] == "lit":
            w.code(*ll[t[1]])
        elif t[0] == "match":
            s, e, x = length_symbol(t[1], len(t) > 3 and t[3])
            w.code(*ll[s]); w.put(x, e)
            s, e, x = dist_symbol(t[2])
            w.code(*d[s]); w.put(x, e)
        elif t[0] == "ll":
            w.code(*ll[t[1]])
        elif t[0] == "d":
            w.code(*d[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        elif t[0] == "eob":
            w.code(*ll[256])
        else:
            raise ValueError(t)


def fixed_block(w, symbols, final=True, eob=True):
    w.put(1 if final else 0, 1); w.put(1, 2)
    put_symbols(w, FIXED_LL, FIXED_D, list(symbols) + ([("eob",)] if eob else []))


def stored_block(w, data, final=True, nlen_xor=0):
    w.put(1 if final else 0, 1); w.put(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) ^ nlen_xor) + data)


def plain_tokens(lens):
    return [(ln,) for ln in lens]


def rle_tokens(lens):
    """greedy run-length tokens over the whole sequence (literal/length and distance lengths as one: runs cross the seam)"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take - 11) if take >= 11 else (17, take - 3))
        elif v != 0 and run >= 4:
            take = 1 + min(run - 1, 6)
            out += [(v,), (16, take - 1 - 3)]
        else:
            take = 1
            out.append((v,))
        i += take
    return out


def expand_tokens(tokens):
    out = []
    for t in tokens:
        if t[0] < 16:
            out.append(t[0])
        elif t[0] == 16:
            out += [out[-1]] * (3 + t[1])
        elif t[0] == 17:
            out += [0] * (3 + t[1])
        else:
            out += [0] * (11 + t[1])
    return out


CL_ALL = {s: (4 if i < 13 else 5) for i, s in enumerate(range(19))}                  # complete: 13 / 16 + 6 / 32
CL_EIGHT = {s: 3 for s in (16, 17, 18, 0, 8, 7, 9, 6)}                              # complete, HCLEN field 4


def dynamic_block(w, ll_lens, d_lens, symbols, final=True, tokens=None, cl=None, n_cl=None, check=True, eob=True):
    """a dynamic block: HLIT = len(ll_lens), HDIST = len(d_lens); tokens: the code-length symbols [(0..15,) | (16|17|18, extra)]
    (default: one per length); cl: {symbol: length} of the code-length code (default: all nineteen); n_cl: how many of them are
    written (default: up to the last non-zero one in the RFC's order)"""
    cl = CL_ALL if cl is None else cl
    tokens = plain_tokens(list(ll_lens) + list(d_lens)) if tokens is None else tokens
    if check:
        assert expand_tokens(tokens) == list(ll_lens) + list(d_lens)
    cl_lens = [cl.get(s, 0) for s in range(19)]
    if n_cl is None:
        n_cl = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    w.put(1 if final else 0, 1); w.put(2, 2)
    w.put(len(ll_lens) - 257, 5); w.put(len(d_lens) - 1, 5); w.put(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        w.put(cl_lens[s], 3)
    cc = canonical(cl_lens)
    for t in tokens:
        w.code(*cc[t[0]])
        if t[0] >= 16:
            w.put(t[1], {16: 2, 17: 3, 18: 7}[t[0]])
    ll, d = canonical(ll_lens), canonical(d_lens)
    put_symbols(w, ll, d, list(symbols) + ([("eob",)] if eob else []))


def lens_for(assign, n):
    """{symbol: length} -> a list of n lengths"""
    out = [0] * n
    for s, ln in assign.items():
        out[s] = ln
    return out


def apply_symbols(symbols, before=b""):
    """the bytes a symbol list stands for (the checker of the crafted entries' `data`)"""
    out = bytearray(before)
    for t in symbols:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out[len(before):])


def _z(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[flush_at:]) + co.flush()


def _valid(name, payload, data):
    return Entry(name, bytes(payload), bytes(data), len(data), zlib.crc32(data) & 0xFFFFFFFF, 0, False)


def _damaged(name, payload, bit, isize=16, crc=0, stream=True):
    return Entry(name, bytes(payload), None, isize, crc, bit, stream)


def _text(rng, n):
    words = [b"ACGT", b"GATTACA", b"chr7", b"\x00\x00\x10\x00", b"\xff" * 5, b"SA:Z:", b"read/", b"TTAGGG"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words)
        if rng.random() < 0.3:
            out += bytes([rng.randrange(256)])
    return bytes(out[:n])


def corpus():
    rng = random.Random(20240613)
    rnd = lambda n: bytes(rng.getrandbits(8) for _ in range(n))                      # noqa: E731
    E = []
    # ---------------------------------------------------------------- from zlib's compressor
    text = _text(rng, 40000)
    E.append(_valid("zlib level 0: stored", _z(text[:5000], 0), text[:5000]))
    E.append(_valid("zlib Z_FIXED", _z(text[:9000], 6, zlib.Z_FIXED), text[:9000]))
    E.append(_valid("zlib level 6: dynamic", _z(text, 6), text))
    E.append(_valid("zlib level 9: dynamic", _z(text[:33333], 9), text[:33333]))
    mixed = b"".join(_text(rng, 3000) + rnd(1500) for _ in range(14))[:65280]
    E.append(_valid("zlib memLevel 1: several dynamic blocks", _z(mixed, 6, mem=1), mixed))
    E.append(_valid("zlib Z_HUFFMAN_ONLY", _z(text[:20001], 6, zlib.Z_HUFFMAN_ONLY), text[:20001]))
    runs = b"".join(bytes([rng.randrange(4)]) * rng.randrange(1, 400) for _ in range(200))[:30011]
    E.append(_valid("zlib Z_RLE", _z(runs, 6, zlib.Z_RLE), runs))
    E.append(_valid("zlib Z_FULL_FLUSH in mid-stream", _z(text[:7001], 6, flush_at=3333), text[:7001]))
    for n in (0, 1, 2, 3):
        E.append(_valid("zlib %d byte(s)" % n, _z(text[:n], 6), text[:n]))
    far = rnd(32768)
    far += far[:300]
    E.append(_valid("zlib match at distance 32768", _z(far, 9), far))
    E.append(_valid("zlib 65536 bytes of one value", _z(b"\x41" * 65536, 6), b"\x41" * 65536))
    big = rnd(65536)
    E.append(_valid("zlib level 0, 65536 random bytes: two stored blocks", _z(big, 0), big))
    E.append(_valid("zlib payload followed by 7 garbage bytes", _z(text[:1234], 6) + b"\xde\xad\xbe\xef\x01\x02\x03", text[:1234]))
    # ---------------------------------------------------------------- crafted, valid
    def fixed(name, symbols, before_symbols=()):
        w = Bits()
        fixed_block(w, list(before_symbols) + list(symbols))
        E.append(_valid(name, w.bytes(), apply_symbols(list(before_symbols) + list(symbols))))

    fixed("fixed literals 0 143 144 255", [("lit", v) for v in (0, 143, 144, 255)])
    seed = [("lit", v) for v in b"abcdefghij"]
    for ln in (3, 10, 11, 257, 258):
        fixed("fixed length %d" % ln, seed + [("match", ln, 10)])
    fixed("fixed length 258 as symbol 284 + 31", seed + [("match", 258, 10, True)])
    block = [("lit", v) for v in rnd(70)]
    for dist in (1, 2, 63, 64, 65):
        fixed("fixed distance %d" % dist, block + [("match", 40, dist)])
    for dist, ln in ((1, 63), (1, 64), (1, 65), (3, 64), (63, 64), (63, 200), (64, 65), (64, 258), (65, 64), (65, 66), (65, 258)):
        fixed("fixed distance %d < length %d" % (dist, ln) if dist < ln else "fixed distance %d, length %d" % (dist, ln), block + [("match", ln, dist)])
    for dist in (24577, 32768):
        w = Bits()
        head = rnd(32768)
        stored_block(w, head, final=False)
        fixed_block(w, [("match", 258, dist), ("lit", 7), ("match", 5, dist)])
        E.append(_valid("stored then fixed distance %d" % dist, w.bytes(), head + apply_symbols([("match", 258, dist), ("lit", 7), ("match", 5, dist)], head)))
    # a match that reaches back across a deflate-block boundary (fixed -> fixed, and dynamic -> stored -> fixed)
    w = Bits()
    first = [("lit", v) for v in b"0123456789"]
    fixed_block(w, first, final=False)
    second = [("match", 9, 10), ("lit", 33), ("match", 30, 3)]
    fixed_block(w, second)
    d0 = apply_symbols(first)
    E.append(_valid("match across a block boundary", w.bytes(), d0 + apply_symbols(second, d0)))
    # dynamic blocks
    lit64 = lens_for({**{v: 6 for v in range(63)}, 256: 6}, 257)                      # 64 codes of 6 bits: complete; HLIT 257
    msg = [("lit", v) for v in (rng.randrange(63) for _ in range(500))]
    w = Bits()
    dynamic_block(w, lit64, [0], msg, tokens=rle_tokens(lit64 + [0]), cl=CL_EIGHT)
    E.append(_valid("dynamic, 8 code-length codes (HCLEN field 4), HLIT 257, no distance code", w.bytes(), apply_symbols(msg)))
    w = Bits()
    dynamic_block(w, lit64, [0], msg[:77], n_cl=19)
    E.append(_valid("dynamic, 19 code-length codes, literals only", w.bytes(), apply_symbols(msg[:77])))
    w = Bits()
    run = [("lit", 5), ("match", 258, 1), ("match", 3, 1), ("lit", 9), ("match", 258, 1)]
    lit_m = lens_for({**{v: 6 for v in range(61)}, 256: 6, 257: 6, 285: 6}, 286)      # 61 literals, end of block, lengths 3 and 258
    dynamic_block(w, lit_m, [1], run, tokens=rle_tokens(lit_m + [1]))
    E.append(_valid("dynamic, one distance code of length 1", w.bytes(), apply_symbols(run)))
    # a 15-bit code: lengths 1 .. 15 and a second 15
    ladder = lens_for({**{65 + k: k + 2 for k in range(14)}, 256: 1, 80: 15}, 257)
    assert sum(2.0 ** -v for v in ladder if v) == 1.0
    deep = [("lit", 65 + k) for k in range(14)] + [("lit", 80), ("lit", 78), ("lit", 80)]
    w = Bits()
    dynamic_block(w, ladder, [0], deep, tokens=rle_tokens(ladder + [0]))
    E.append(_valid("dynamic, 15-bit codes", w.bytes(), apply_symbols(deep)))
    # ... and 15-bit distance codes
    dl = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]
    lens_m = lens_for({**{v: 7 for v in range(100, 163)}, 256: 7, **{257 + k: 7 for k in range(29)}, **{v: 7 for v in range(35)}}, 286)
    assert sum(2.0 ** -v for v in lens_m if v) == 1.0
    pre = [("lit", v) for v in list(range(100, 163)) * 5]
    deepd = pre + [("match", 20, 250), ("match", 7, 255), ("match", 258, 130), ("lit", 3), ("match", 4, 1)]
    w = Bits()
    dynamic_block(w, lens_m, dl, deepd, tokens=rle_tokens(lens_m + dl))
    E.append(_valid("dynamic, 15-bit distance codes", w.bytes(), apply_symbols(deepd)))
    # repeat codes at their minimum and maximum counts; lengths 8: 256 symbols complete
    def repeats(name, ll_lens, d_lens, tokens, symbols):
        w = Bits()
        dynamic_block(w, ll_lens, d_lens, symbols, tokens=tokens)
        E.append(_valid(name, w.bytes(), apply_symbols(symbols)))

    # 16: 6 and 3 copies; 17: 3 and 10 zeros; 18: 11 and 138 zeros.  4 codes of 6 bits and 120 of 7: complete
    ll = [6] * 4 + [7] * 7 + [0] * 3 + [7] * 4 + [0] * 10 + [7] * 2 + [0] * 11 + [7] + [0] * 138 + [7] * 106
    tok = ([(6,)] * 4 + [(7,), (16, 3)] + [(17, 0)] + [(7,), (16, 0)] + [(17, 7)] + [(7,)] * 2 + [(18, 0)] + [(7,)] + [(18, 127)] + [(7,)] * 106)
    dl = [4] * 14 + [5] * 4
    assert len(ll) == 286 and ll[256] and sum(2.0 ** -v for v in ll if v) == 1.0 and sum(2.0 ** -v for v in dl) == 1.0
    body = [("lit", s) for s, v in enumerate(ll[:256]) if v] * 2 + [("match", 17, 9), ("match", 258, 100)]
    repeats("dynamic, repeat codes at minimum and maximum counts", ll, dl, tok + plain_tokens(dl), body)
    # a repeat that crosses from the literal/length lengths into the distance lengths: the 16 behind length 258 writes 259 and four distances
    ll2 = [8] * 100 + [0] * 4 + [8] * 156
    dl2 = [8, 8, 8, 8, 6, 5, 4, 3, 2, 1]
    assert len(ll2) == 260 and sum(2.0 ** -v for v in dl2) == 1.0 and sum(2.0 ** -v for v in ll2 if v) == 1.0
    tok2 = plain_tokens(ll2[:259]) + [(16, 2)] + plain_tokens(dl2[4:])
    body2 = [("lit", v) for v in range(40)] + [("match", 3, 3), ("match", 5, 30), ("match", 4, 9)]
    repeats("dynamic, a repeat crosses into the distance lengths", ll2, dl2, tok2, body2)
    # ... and a run of zeros (18) that does: 12 literal/length lengths and 3 distance lengths
    ll3 = lens_for({**{v: 6 for v in range(62)}, 256: 6, 257: 6}, 270)
    dl3 = [0, 0, 0, 1]
    tok3 = plain_tokens(ll3[:258]) + [(18, 15 - 11)] + [(1,)]
    body3 = [("lit", v) for v in range(30)] + [("match", 3, 4), ("match", 3, 4)]
    repeats("dynamic, a run of zeros crosses into the distance lengths", ll3, dl3, tok3, body3)
    # a symbol whose code straddles bit 32 and bit 64 of the payload: 3 header bits, 8-bit literals, then a 9-bit one
    w = Bits()
    strad = [("lit", 1), ("lit", 2), ("lit", 3), ("lit", 200), ("lit", 4), ("lit", 5), ("lit", 6), ("lit", 250), ("lit", 9)]
    fixed_block(w, strad)
    assert 3 + 24 < 32 < 3 + 24 + 9 and 3 + 24 + 9 + 24 < 64 < 3 + 24 + 9 + 24 + 9
    E.append(_valid("fixed, codes straddle bit 32 and bit 64", w.bytes(), apply_symbols(strad)))
    # an empty stored block at the end, after the output is complete
    w = Bits()
    fixed_block(w, seed, final=False)
    stored_block(w, b"")
    E.append(_valid("fixed then an empty final stored block", w.bytes(), apply_symbols(seed)))
    # ---------------------------------------------------------------- crafted, damaged: one status bit each
    w = Bits(); w.put(1, 1); w.put(3, 2); w.put(0, 13)
    E.append(_damaged("block type 3", w.bytes(), E_HEADER))
    w = Bits(); stored_block(w, b"sixteen bytes...", nlen_xor=1)
    E.append(_damaged("stored NLEN wrong", w.bytes(), E_HEADER))
    w = Bits(); dynamic_block(w, lens_for({0: 1, 1: 1, 256: 1}, 257), [0], [("lit", 0)] * 16, check=True)
    E.append(_damaged("dynamic, over-subscribed lengths", w.bytes(), E_LENGTHS))
    w = Bits(); dynamic_block(w, lens_for({65: 2, 256: 2}, 257), [0], [("lit", 65)] * 16)
    E.append(_damaged("dynamic, incomplete literal/length set", w.bytes(), E_LENGTHS))
    w = Bits(); dynamic_block(w, lens_for({0: 1, 1: 1}, 257), [0], [("lit", 0)] * 16, eob=False)
    E.append(_damaged("dynamic, no code for 256", w.bytes(), E_LENGTHS))
    w = Bits(); dynamic_block(w, [0] * 257, [0], [], tokens=[(18, 127), (18, 120 - 11)], cl={16: 2, 17: 2, 18: 2, 0: 2}, n_cl=4, eob=False)
    E.append(_damaged("dynamic, 4 code-length codes: only zeros", w.bytes(), E_LENGTHS))
    w = Bits(); dynamic_block(w, lit64, [0], [("lit", 0)] * 16, tokens=[(16, 0)] + plain_tokens(lit64[3:] + [0]), check=False)
    E.append(_damaged("dynamic, code 16 first", w.bytes(), E_SYMBOL))
    for s in (286, 287):
        w = Bits(); fixed_block(w, seed + [("ll", s)] + seed)
        E.append(_damaged("fixed, symbol %d" % s, w.bytes(), E_SYMBOL, isize=20))
    w = Bits(); fixed_block(w, seed + [("ll", 257), ("d", 30)] + seed)
    E.append(_damaged("fixed, distance code 30", w.bytes(), E_SYMBOL, isize=23))
    w = Bits(); fixed_block(w, seed[:3] + [("match", 3, 4)] + seed)
    E.append(_damaged("distance one beyond the bytes produced", w.bytes(), E_DISTANCE))
    data = text[100:2100]
    E.append(Entry("a stream one byte longer than ISIZE", _z(data + b"x", 6), None, len(data), zlib.crc32(data) & 0xFFFFFFFF, E_OUTPUT, False))
    E.append(Entry("a stream one byte shorter than ISIZE", _z(data[:-1], 6), None, len(data), zlib.crc32(data) & 0xFFFFFFFF, E_SHORT, False))
    w = Bits(); fixed_block(w, seed)
    E.append(_damaged("a payload cut in mid-symbol", w.bytes()[:2], E_INPUT, isize=10))
    E.append(Entry("a correct stream with a wrong CRC", _z(data, 6), None, len(data), (zlib.crc32(data) ^ 0x00010000) & 0xFFFFFFFF, E_CRC, False))
    return E


def write_corpus(path, entries):
    """the corpus file tests/inflate_core_main.cpp reads: u32 count, then per entry u32 payload bytes, u32 isize, u32 crc, payload"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(entries)))
        for e in entries:
            f.write(struct.pack("<III", len(e.payload), e.isize, e.crc) + e.payload)
