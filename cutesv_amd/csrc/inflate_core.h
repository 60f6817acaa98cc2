// inflate_core.h — a raw-DEFLATE (RFC 1951) decoder for one BGZF block, written once for the host and for the device
// (DESIGN.md section 27).  Plain C++: no HIP header, no global state.  The code is templated on a `Lanes` policy that says how
// many lanes execute it together:
//   InfOneLane (below)      the host form: one lane.  It is the statement of the contract of csv_bgzf_inflate, and what
//                           tests/inflate_core_main.cpp runs under the address and undefined-behaviour sanitizers.
//   InfWave (bam.hip.h)     the device form: the 64 lanes of a wavefront.  Everything that decides - the bit reader, the
//                           code-length parser, the symbol loop, the status rules - runs redundantly in every lane on values
//                           made wave-uniform (Lanes::uni), so every decision to leave a block is taken by all lanes alike; the
//                           lanes differ only in the strided loops (table build, stored block, match copy) and inside Lanes::crc.
// What a Lanes type provides: lane(), width(), uni(uint32_t) (the value of the first lane), sync() (the writes of every lane
// to the tables and to `out` are visible to every lane afterwards), crc(out, len, table) (the finished CRC32 of out[0 .. len)).
//
// Bounds, by construction (section 27 has the argument in full):
//   * a byte of the payload is read only by InfBits::word, at an index it has compared with `n`; behind the payload it
//     delivers zero bits.  After every code the consumed bits are compared with 8 n: beyond -> INF_E_INPUT, the block is left.
//     Every code consumes at least one bit, so the symbol loop ends after at most 8 n + 1 rounds.
//   * a byte of `out` is written only at an index below out_len (a literal at opos < out_len, a match or a stored block after
//     opos + len <= out_len) and read only below opos: the window is the block's own output and nothing else.
//   * table indices: a code length is at most 15, a symbol index is compared with the table's size before it is used.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define INF_FN __host__ __device__ inline
#else
#define INF_FN inline
#endif

namespace csv {

// csv_bgzf_inflate's status bits (mirrored as CSV_INF_E_* in include/cutesv_hip.h)
enum {
    INF_E_HEADER = 1,       // block type 3, or a stored block whose LEN and NLEN do not complement each other
    INF_E_LENGTHS = 2,      // over-subscribed or incomplete code lengths, too many of them, or no end-of-block code
    INF_E_SYMBOL = 4,       // literal/length 286 / 287, distance 30 / 31, a repeat with nothing before it, a bit pattern that is no code
    INF_E_DISTANCE = 8,     // a distance beyond the bytes produced so far in this BGZF block
    INF_E_OUTPUT = 16,      // the output would pass out_len
    INF_E_SHORT = 32,       // the final block ended short of out_len
    INF_E_INPUT = 64,       // the payload ended inside the stream
    INF_E_CRC = 128         // everything decoded, and the CRC32 differs
};

constexpr int INF_LL_SYMS = 288, INF_LL_FAST = 9, INF_D_SYMS = 32, INF_D_FAST = 7;

// a canonical Huffman code: cnt[l] codes of length l, sym = the symbols in code order, fast[bits] = symbol << 4 | length for
// the codes of at most FAST bits (0: a longer code, or none)
template <int NSYM, int FAST> struct InfHuff {
    uint16_t cnt[16];
    uint16_t sym[NSYM];
    uint16_t fast[1 << FAST];
};
// what one decoder needs beside its registers: 1632 + 352 + 320 bytes
struct InfWork {
    InfHuff<INF_LL_SYMS, INF_LL_FAST> ll;
    InfHuff<INF_D_SYMS, INF_D_FAST> d;       // the distance code; while a dynamic header is read, the code-length code
    uint8_t len[INF_LL_SYMS + INF_D_SYMS];   // code lengths: literal/length, then distance
};

struct InfOneLane {
    INF_FN int lane() const { return 0; }
    INF_FN int width() const { return 1; }
    INF_FN uint32_t uni(uint32_t v) const { return v; }
    INF_FN void sync() const {}
    INF_FN uint32_t crc(const uint8_t* out, int32_t len, const uint32_t* table) const
    {
        uint32_t c = 0xffffffffu;
        for (int32_t i = 0; i < len; i++) c = table[(c ^ out[i]) & 255u] ^ (c >> 8);
        return c ^ 0xffffffffu;
    }
};

// entry i of the CRC32 table (reflected polynomial 0xEDB88320)
INF_FN uint32_t inf_crc_entry(uint32_t i)
{
    for (int k = 0; k < 8; k++) i = (i >> 1) ^ ((i & 1u) ? 0xEDB88320u : 0u);
    return i;
}

// ---- the bit reader: `cnt` valid bits at the bottom of `buf`, the next payload byte to fetch is `pos`
template <class Lanes> struct InfBits {
    const uint8_t* p;
    int64_t n, pos;
    uint64_t buf;
    int cnt;
    Lanes L;

    INF_FN uint32_t word(int64_t at) const       // payload bytes [at, at + 4), zeros behind the payload
    {
        uint32_t w = 0;
        if (at + 4 <= n) memcpy(&w, p + at, 4);
        else
            for (int k = 0; k < 4; k++)
                if (at + k < n) w |= (uint32_t)p[at + k] << (8 * k);
        return L.uni(w);
    }
    INF_FN void refill()                         // afterwards cnt >= 33
    {
        if (cnt <= 32) { buf |= (uint64_t)word(pos) << cnt; cnt += 32; pos += 4; }
    }
    INF_FN uint32_t peek(int k) const { return (uint32_t)buf & ((1u << k) - 1u); }            // k <= 16 <= cnt
    INF_FN void drop(int k) { buf >>= k; cnt -= k; }
    INF_FN uint32_t take(int k) { const uint32_t v = peek(k); drop(k); return v; }
    INF_FN int64_t consumed() const { return 8 * pos - cnt; }
    INF_FN bool over() const { return consumed() > 8 * n; }
    INF_FN bool fewer_than(int k) const { return 8 * n - consumed() < k; }      // fewer than k real bits are left
};

// the symbol of the code at the bottom of `bits` (first bit of the stream lowest), looking at lengths 1 .. maxlen:
// symbol << 4 | length, or 0 when no code of those lengths matches
template <int NSYM, int FAST> INF_FN uint32_t inf_slow(const InfHuff<NSYM, FAST>& H, uint32_t bits, int maxlen)
{
    int code = 0, first = 0, index = 0;
#pragma GCC unroll 1
    for (int len = 1; len <= maxlen; len++) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = H.cnt[len];
        if (code - c < first) {
            const int at = index + (code - first);
            return at < NSYM ? ((uint32_t)H.sym[at] << 4) | (uint32_t)len : 0u;
        }
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return 0u;
}

// the tables of the code with lengths len[0 .. n).  Returns 0, or INF_E_LENGTHS: over-subscribed, or incomplete where zlib
// refuses that (`strict`: always; else unless the longest code has one bit or there is no code at all).
template <class Lanes, int NSYM, int FAST> INF_FN int inf_build(const Lanes& L, InfHuff<NSYM, FAST>& H, const uint8_t* len, int n, bool strict)
{
    L.sync();                                                     // (the lengths are in place; nobody still reads the old tables)
    for (int l = L.lane(); l < 16; l += L.width()) {
        int c = 0;
#pragma GCC unroll 1
        for (int s = 0; s < n; s++) c += len[s] == l;
        H.cnt[l] = (uint16_t)c;
    }
    L.sync();
    int left = 1, longest = 0;
    for (int l = 1; l < 16; l++) {
        const int c = (int)L.uni(H.cnt[l]);
        left = 2 * left - c;
        if (left < 0) return INF_E_LENGTHS;
        if (c) longest = l;
    }
    if (left > 0 && (strict || longest > 1)) return INF_E_LENGTHS;
    for (int l = 1 + L.lane(); l < 16; l += L.width()) {          // the symbols of length l, in symbol order, behind those of the shorter lengths
        int o = 0;
#pragma GCC unroll 1
        for (int k = 1; k < l; k++) o += H.cnt[k];
#pragma GCC unroll 1
        for (int s = 0; s < n; s++)
            if (len[s] == l && o < NSYM) H.sym[o++] = (uint16_t)s;
    }
    L.sync();
#pragma GCC unroll 1
    for (int i = L.lane(); i < (1 << FAST); i += L.width()) H.fast[i] = (uint16_t)inf_slow(H, (uint32_t)i, FAST);
    L.sync();
    return 0;
}

// the next symbol of the stream: symbol << 4 | length with the bits consumed, or 0 (no code matches the next 15 bits)
template <class Lanes, int NSYM, int FAST> INF_FN uint32_t inf_symbol(InfBits<Lanes>& B, const InfHuff<NSYM, FAST>& H)
{
    B.refill();
    uint32_t e = B.L.uni(H.fast[B.peek(FAST)]);
    if (!e) e = B.L.uni(inf_slow(H, B.peek(15), 15));
    B.drop((int)(e & 15u));
    return e;
}

INF_FN int inf_len_base(int s)  { return s < 8 ? 3 + s : s == 28 ? 258 : ((4 + (s & 3)) << ((s >> 2) - 1)) + 3; }      // s = symbol - 257
INF_FN int inf_len_extra(int s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
INF_FN int inf_dist_base(int s) { return s < 4 ? 1 + s : ((2 + (s & 1)) << ((s >> 1) - 1)) + 1; }
INF_FN int inf_dist_extra(int s) { return s < 4 ? 0 : (s >> 1) - 1; }

// the code lengths of a dynamic block's header -> W.len and both tables.  0, or one status bit.
template <class Lanes> INF_FN int inf_dynamic(InfBits<Lanes>& B, InfWork& W)
{
    const Lanes& L = B.L;
    B.refill();
    const int nlen = (int)B.take(5) + 257, ndist = (int)B.take(5) + 1, ncode = (int)B.take(4) + 4;
    if (B.over()) return INF_E_INPUT;
    if (nlen > 286 || ndist > 30) return INF_E_LENGTHS;
    uint8_t* cl = W.len + INF_LL_SYMS;                             // the 19 lengths of the code-length code borrow the distance lengths' place
    L.sync();
    for (int i = 0; i < 19; i++) {                                 // in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        B.refill();
        const int v = i < ncode ? (int)B.take(3) : 0;
        const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) / 2 : 8 + (i - 4) / 2;
        if (L.lane() == 0) cl[at] = (uint8_t)v;
    }
    if (B.over()) return INF_E_INPUT;
    if (inf_build(L, W.d, cl, 19, true)) return INF_E_LENGTHS;     // (built: cl is free again)
    const int total = nlen + ndist;
    int have = 0, prev = 0;
    while (have < total) {                                         // every round consumes at least one bit or leaves, and `have` grows
        const uint32_t e = inf_symbol(B, W.d);
        if (B.over()) return INF_E_INPUT;
        if (!e) return B.fewer_than(15) ? INF_E_INPUT : INF_E_SYMBOL;
        const int s = (int)(e >> 4);
        int rep = 1, val = s;
        if (s >= 16) {
            B.refill();
            if (s == 16) { if (have == 0) return INF_E_SYMBOL; val = prev; rep = 3 + (int)B.take(2); }
            else if (s == 17) { val = 0; rep = 3 + (int)B.take(3); }
            else { val = 0; rep = 11 + (int)B.take(7); }
            if (B.over()) return INF_E_INPUT;
            if (have + rep > total) return INF_E_LENGTHS;
        }
        // literal/length lengths at len[0 .. nlen), distance lengths at len[INF_LL_SYMS ..): a repeat may run from one into the other
        for (int i = L.lane(); i < rep; i += L.width()) {
            const int at = have + i;
            W.len[at < nlen ? at : INF_LL_SYMS + (at - nlen)] = (uint8_t)val;
        }
        have += rep; prev = val;
    }
    L.sync();
    if (L.uni(W.len[256]) == 0) return INF_E_LENGTHS;
    if (inf_build(L, W.ll, W.len, nlen, false)) return INF_E_LENGTHS;
    if (inf_build(L, W.d, cl, ndist, false)) return INF_E_LENGTHS;
    return 0;
}

template <class Lanes> INF_FN void inf_fixed(const Lanes& L, InfWork& W)
{
    L.sync();
    for (int i = L.lane(); i < INF_LL_SYMS + INF_D_SYMS; i += L.width())
        W.len[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    (void)inf_build(L, W.ll, W.len, INF_LL_SYMS, false);
    (void)inf_build(L, W.d, W.len + INF_LL_SYMS, INF_D_SYMS, false);
}

// One BGZF block: the raw-deflate payload p[0 .. n) -> out[0 .. out_len).  Returns the status byte: 0 means out holds what
// zlib's inflate gives and its CRC32 is `crc`.  crc_table: the 256 entries of inf_crc_entry.
template <class Lanes> INF_FN int inf_block(const Lanes& L, InfWork& W, const uint8_t* p, int32_t n, uint8_t* out, int32_t out_len, uint32_t crc, const uint32_t* crc_table)
{
    InfBits<Lanes> B{p, (int64_t)n, 0, 0, 0, L};
    int32_t opos = 0;
    for (;;) {                                                     // deflate blocks: each consumes at least its 3 header bits
        B.refill();
        const int last = (int)B.take(1), type = (int)B.take(2);
        if (B.over()) return INF_E_INPUT;
        if (type == 3) return INF_E_HEADER;
        if (type == 0) {
            B.drop(B.cnt & 7);                                     // to the byte boundary (8 pos is one, so cnt tells)
            B.refill();
            const uint32_t len = B.take(16);
            B.refill();
            const uint32_t nlen = B.take(16);
            if (B.over()) return INF_E_INPUT;
            if ((len ^ nlen) != 0xffffu) return INF_E_HEADER;
            const int64_t src = B.consumed() >> 3;
            if (src + (int64_t)len > B.n) return INF_E_INPUT;
            if ((int64_t)opos + (int64_t)len > (int64_t)out_len) return INF_E_OUTPUT;
#pragma GCC unroll 1
            for (int32_t i = L.lane(); i < (int32_t)len; i += L.width()) out[opos + i] = p[src + i];
            L.sync();
            opos += (int32_t)len;
            B.pos = src + (int64_t)len; B.buf = 0; B.cnt = 0;
        } else {
            if (type == 1) inf_fixed(L, W);
            else { const int st = inf_dynamic(B, W); if (st) return st; }
            for (;;) {                                             // symbols: each consumes at least one bit, or the block is left
                const uint32_t e = inf_symbol(B, W.ll);
                if (B.over()) return INF_E_INPUT;
                if (!e) return B.fewer_than(15) ? INF_E_INPUT : INF_E_SYMBOL;
                const int s = (int)(e >> 4);
                if (s < 256) {
                    if (opos >= out_len) return INF_E_OUTPUT;
                    if (L.lane() == 0) out[opos] = (uint8_t)s;
                    opos++;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return INF_E_SYMBOL;
                const int len = inf_len_base(s - 257) + (int)B.take(inf_len_extra(s - 257));
                const uint32_t ed = inf_symbol(B, W.d);
                if (B.over()) return INF_E_INPUT;
                if (!ed) return B.fewer_than(15) ? INF_E_INPUT : INF_E_SYMBOL;
                const int ds = (int)(ed >> 4);
                if (ds > 29) return INF_E_SYMBOL;
                const int dist = inf_dist_base(ds) + (int)B.take(inf_dist_extra(ds));
                if (B.over()) return INF_E_INPUT;
                if (dist > opos) return INF_E_DISTANCE;
                if (opos + len > out_len) return INF_E_OUTPUT;
                // byte i of the match is byte i mod dist of the `dist` bytes before it: every source lies below opos
                L.sync();
                const uint8_t* from = out + (opos - dist);
#pragma GCC unroll 1
                for (int i = L.lane(); i < len; i += L.width()) out[opos + i] = from[dist >= len ? i : i % dist];
                L.sync();
                opos += len;
            }
        }
        if (last) break;
    }
    if (opos < out_len) return INF_E_SHORT;
    L.sync();
    return L.crc(out, out_len, crc_table) == crc ? 0 : INF_E_CRC;
}

}  // namespace csv
