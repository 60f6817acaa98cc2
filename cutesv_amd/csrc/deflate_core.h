// deflate_core.h — a DEFLATE (RFC 1951) compressor for one BGZF block, written once for the host and for the device (DESIGN.md
// section 34).  Plain C++: no HIP header, no global state; the style of inflate_core.h.  The code is templated on a `Lanes` policy:
//   DflOneLane (below)      the host form: one lane, which walks the 64 positions of a tile one after the other.  It states the
//                           contract of csv_bgzf_deflate (csv_bgzf_deflate_host runs it) and is what tests/deflate_core_main.cpp
//                           runs under the address and undefined-behaviour sanitizers.
//   DflWave (bam.hip.h)     the device form: the 64 lanes of a wavefront, one lane per position of a tile.
// What a Lanes type provides beside inflate_core.h's (lane, width, uni, sync, crc): amax / add / or32 (on a word of the work area:
// the maximum, the sum, the bitwise or - results that do not depend on the order of arrival), ballot_nz(a) (bit l: a[l] != 0,
// l < 64), scan64(a) (a[0 .. 64) -> its exclusive prefix sums in place; returns the total).
//
// dfl_block: in[0 .. n), 0 <= n <= 65280 -> one complete BGZF block in out[0 .. 65536): the 18-byte header with the BC field and
// BSIZE, a raw-DEFLATE payload of ONE final deflate block, CRC32 and ISIZE.  Returns the block's size, at most n + 31 (the stored form).
//
// THE OUTPUT IS A PURE FUNCTION OF THE INPUT.  Nothing depends on which lane comes first:
//   * the parse works on tiles of 64 positions.  A position's candidate is read from the hash table AS IT STOOD BEFORE THE TILE
//     (read, wavefront barrier, then insert), so a match source always lies in an earlier tile;
//   * the tile's positions enter the table with "largest position wins" (amax);
//   * the greedy, non-overlapping choice is a walk over the ballot of the lanes that hold a match, in lane order, on wave-uniform
//     values: every lane computes the same `starts` mask;
//   * histogram counts are sums, the staged bits of a tile are or-ed into disjoint bit ranges.
// Tokens: one 32-bit word PER INPUT POSITION in `tok` (0: covered by an earlier match) - a slot of device scratch per wavefront,
// a heap block on the host - so one deflate block and one set of code tables serve the whole BGZF block.
//
// Bounds, by construction:
//   * an input byte is read at p + k only after p + k (+ width of the load) <= n was compared: the hash at p + 4 <= n, dfl_match
//     below maxlen <= n - p; a match source c < p reads c + k < p + k.
//   * `out` is written through DflBits::word (index compared with 16384 words) and dfl_byte (index compared with 65536); the size of the
//     coding that is written was computed before and is at most the stored form's n + 31 <= 65311.
//   * tok[p] only for p < n; every table index is compared with its table's size (symbols by arithmetic: length symbol <= 285,
//     distance symbol <= 29, and clamped where they index), the staging words with DFL_STAGE.
#pragma once
#include <stdint.h>
#include <string.h>

#include "inflate_core.h"

namespace csv {

constexpr int DFL_MAX_IN = 65280, DFL_SLOT = 65536, DFL_TILE = 64;
constexpr int DFL_HASH_BITS = 12, DFL_MIN_MATCH = 4, DFL_MAX_MATCH = 258, DFL_MAX_DIST = 32768, DFL_FAR = 4096;
constexpr int DFL_LL = 286, DFL_D = 30, DFL_CL = 19, DFL_SEQ = 320, DFL_STAGE = 128;
enum { DFL_STORED = 0, DFL_FIXED = 1, DFL_DYNAMIC = 2 };
constexpr uint32_t DFL_TOK = 0x80000000u, DFL_TOK_MATCH = 0x40000000u;       // literal: TOK | byte; match: TOK | MATCH | (len - 3) << 16 | (dist - 1)

// what one compressor needs beside its registers and its token slot: about 22 KiB (LDS on the device)
struct DflWork {
    uint32_t hash[1 << DFL_HASH_BITS];       // position + 1 of the last 4 bytes with this hash in front of the tile; 0: none
    uint32_t freq_ll[288], freq_d[32], freq_cl[20];
    uint32_t skey[288];                      // dfl_lengths: the frequencies in ascending order, then the tree in place
    uint16_t ssym[288];
    uint16_t code_ll[288], code_d[32], code_cl[20];      // bit-reversed: the first bit of the stream lowest
    uint16_t seq[DFL_SEQ];                   // the run-length coded code lengths: symbol | extra << 8
    uint16_t tlen[DFL_TILE], tdist[DFL_TILE];            // a tile's matches (0: none)
    uint32_t tnb[DFL_TILE];                  // a tile's bit counts, then their exclusive prefix
    uint32_t stage[DFL_STAGE];               // a tile's bits on their way to `out`
    uint32_t meta[8];                        // hlit, hdist, hclen, entries of seq, header bits
    uint8_t  len_ll[288], len_d[32], len_cl[20];
};

struct DflOneLane : InfOneLane {
    INF_FN void amax(uint32_t* p, uint32_t v) const { if (v > *p) *p = v; }
    INF_FN void add(uint32_t* p, uint32_t v) const { *p += v; }
    INF_FN void or32(uint32_t* p, uint32_t v) const { *p |= v; }
    INF_FN uint64_t ballot_nz(const uint16_t* a) const
    {
        uint64_t m = 0;
        for (int l = 0; l < DFL_TILE; l++) if (a[l]) m |= 1ull << l;
        return m;
    }
    INF_FN uint32_t scan64(uint32_t* a) const
    {
        uint32_t s = 0;
        for (int l = 0; l < DFL_TILE; l++) { const uint32_t v = a[l]; a[l] = s; s += v; }
        return s;
    }
};

INF_FN uint32_t dfl_hash(const uint8_t* p)                        // of p[0 .. 4)
{
    uint32_t w;
    memcpy(&w, p, 4);
    return (w * 2654435761u) >> (32 - DFL_HASH_BITS);
}

// how many bytes agree at in + c and in + p, at most maxlen; c < p, p + maxlen <= n
INF_FN int dfl_match(const uint8_t* in, int32_t c, int32_t p, int maxlen)
{
    int k = 0;
    while (k + 8 <= maxlen) {
        uint64_t a, b;
        memcpy(&a, in + c + k, 8); memcpy(&b, in + p + k, 8);
        const uint64_t x = a ^ b;
        if (x) return k + (__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < maxlen && in[c + k] == in[p + k]) k++;
    return k;
}

// length - 3 in 0 .. 255 -> symbol - 257 and the extra bits (inverse of inf_len_base / inf_len_extra)
INF_FN void dfl_len_sym(int l, int& sym, int& nx, int& x)
{
    if (l < 8) { sym = l; nx = 0; x = 0; return; }
    if (l == 255) { sym = 28; nx = 0; x = 0; return; }
    const int e = (31 - __builtin_clz((unsigned)l)) - 2;
    sym = 4 * (e + 1) + ((l >> e) & 3); nx = e; x = l & ((1 << e) - 1);
}
// distance - 1 in 0 .. 32767 -> symbol and the extra bits
INF_FN void dfl_dist_sym(int d, int& sym, int& nx, int& x)
{
    if (d < 4) { sym = d; nx = 0; x = 0; return; }
    const int hb = 31 - __builtin_clz((unsigned)d), e = hb - 1;
    sym = 2 * hb + ((d >> e) & 1); nx = e; x = d & ((1 << e) - 1);
}

INF_FN uint64_t dfl_span(int a, int b)                             // bits a .. b - 1, 0 <= a < 64, a <= b <= 64
{
    return (b >= 64 ? ~0ull : (1ull << b) - 1) & ~((1ull << a) - 1);
}

// ---- the parse: tok[0 .. n) and the two histograms (the end-of-block symbol included)
template <class Lanes> INF_FN void dfl_parse(const Lanes& L, DflWork& W, const uint8_t* in, int32_t n, uint32_t* tok)
{
    for (int i = L.lane(); i < (1 << DFL_HASH_BITS); i += L.width()) W.hash[i] = 0;
    for (int i = L.lane(); i < 288; i += L.width()) W.freq_ll[i] = i == 256 ? 1u : 0u;
    for (int i = L.lane(); i < 32; i += L.width()) W.freq_d[i] = 0;
    L.sync();
    int32_t next = 0;                                              // the first position no token covers yet (wave-uniform)
    for (int32_t b = 0; b < n; b += DFL_TILE) {
        const bool need = next < b + DFL_TILE;                     // some position of the tile starts a token
        for (int l = L.lane(); l < DFL_TILE; l += L.width()) {
            const int32_t p = b + l;
            int len = 0, dist = 0;
            if (need && p >= next && p + DFL_MIN_MATCH <= n) {
                const uint32_t c1 = W.hash[dfl_hash(in + p)];
                if (c1 && p - (int32_t)(c1 - 1) <= DFL_MAX_DIST) {
                    const int32_t c = (int32_t)(c1 - 1);           // (c < b <= p: it entered the table before this tile)
                    const int room = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
                    len = dfl_match(in, c, p, room); dist = p - c;
                    if (len < DFL_MIN_MATCH || (len == DFL_MIN_MATCH && dist > DFL_FAR)) len = 0;
                }
            }
            W.tlen[l] = (uint16_t)len; W.tdist[l] = (uint16_t)(len ? dist - 1 : 0);
        }
        L.sync();                                                  // every candidate is read: the tile may enter the table
        for (int l = L.lane(); l < DFL_TILE; l += L.width()) {
            const int32_t p = b + l;
            if (p + DFL_MIN_MATCH <= n) L.amax(&W.hash[dfl_hash(in + p)], (uint32_t)p + 1u);
        }
        uint64_t starts = 0;
        if (need) {
            const uint64_t m = L.ballot_nz(W.tlen);
            const int lim = n - b < DFL_TILE ? n - b : DFL_TILE;
            int cur = next > b ? next - b : 0;
            while (cur < lim) {                                    // one round per match of the tile
                const uint64_t mm = m >> cur;
                if (!mm) { starts |= dfl_span(cur, lim); cur = lim; break; }
                const int j = cur + __builtin_ctzll(mm);           // (j < lim: a lane beyond the input holds no match)
                starts |= dfl_span(cur, j + 1);
                const int len = (int)L.uni(W.tlen[j & (DFL_TILE - 1)]);
                cur = j + (len > 0 ? len : 1);                     // (a set bit means len >= DFL_MIN_MATCH; the walk advances whatever it reads)
            }
            next = b + cur;
        }
        for (int l = L.lane(); l < DFL_TILE; l += L.width()) {
            const int32_t p = b + l;
            if (p >= n) continue;
            uint32_t t = 0;
            if ((starts >> l) & 1ull) {
                const int len = W.tlen[l];
                if (len) {
                    int ls, lnx, lx, ds, dnx, dx;
                    dfl_len_sym(len - 3, ls, lnx, lx); dfl_dist_sym(W.tdist[l], ds, dnx, dx);
                    t = DFL_TOK | DFL_TOK_MATCH | ((uint32_t)(len - 3) << 16) | (uint32_t)W.tdist[l];
                    if (ls < 29) L.add(&W.freq_ll[257 + ls], 1u);
                    if (ds < DFL_D) L.add(&W.freq_d[ds], 1u);
                } else {
                    t = DFL_TOK | in[p];
                    L.add(&W.freq_ll[in[p]], 1u);
                }
            }
            tok[p] = t;
        }
        L.sync();
    }
    L.sync();
}

// ---- code lengths: lens[0 .. n) for freq[0 .. n), none above maxbits; a symbol that does not occur gets 0.  The symbols are ranked
// by (frequency, symbol) with all lanes; lane 0 builds the tree in place (Moffat and Katajainen's minimum-redundancy construction)
// and repairs lengths above maxbits on the counts per length (each round takes a code of maxbits away, turns the deepest shorter
// leaf into a node with two leaves: the Kraft sum falls by one unit).  complete: a lone symbol gets a partner, so that the code is
// complete (the code-length code: zlib refuses an incomplete one).  n <= 288.
template <class Lanes> INF_FN void dfl_lengths(const Lanes& L, DflWork& W, const uint32_t* freq, int n, int maxbits, uint8_t* lens, bool complete)
{
    L.sync();
    for (int s = L.lane(); s < n; s += L.width()) {
        lens[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        int r = 0;
#pragma GCC unroll 1
        for (int t = 0; t < n; t++) { const uint32_t g = freq[t]; r += (g != 0 && (g < f || (g == f && t < s))) ? 1 : 0; }
        if (r < 288) { W.skey[r] = f; W.ssym[r] = (uint16_t)s; }
    }
    L.sync();
    if (L.lane() == 0) {
        uint32_t* A = W.skey;
        int m = 0;
        for (int s = 0; s < n; s++) m += freq[s] != 0 ? 1 : 0;
        if (m == 1) {
            const int s = W.ssym[0];
            lens[s] = 1;
            if (complete) lens[s == 0 ? 1 : 0] = 1;
        } else if (m >= 2) {
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int nx = 1; nx < m - 1; nx++) {
                if (leaf >= m || A[root] < A[leaf]) { A[nx] = A[root]; A[root++] = (uint32_t)nx; } else A[nx] = A[leaf++];
                if (leaf >= m || (root < nx && A[root] < A[leaf])) { A[nx] += A[root]; A[root++] = (uint32_t)nx; } else A[nx] += A[leaf++];
            }
            A[m - 2] = 0;
            for (int nx = m - 3; nx >= 0; nx--) A[nx] = A[A[nx] < 288u ? A[nx] : 0u] + 1;
            int avbl = 1, used = 0, dpth = 0;
            root = m - 2;
            int nx = m - 1;
            while (avbl > 0) {
                while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
                while (avbl > used && nx >= 0) { A[nx--] = (uint32_t)dpth; avbl--; }
                if (nx < 0 && avbl > used) break;
                avbl = 2 * used; dpth++; used = 0;
            }
            // A[i]: the depth of the i-th rarest symbol, descending in i
            uint32_t cnt[16];
            for (int l = 0; l < 16; l++) cnt[l] = 0;
            for (int i = 0; i < m; i++) cnt[A[i] < (uint32_t)maxbits ? A[i] : (uint32_t)maxbits]++;
            uint32_t total = 0;
            for (int l = 1; l <= maxbits; l++) total += cnt[l] << (maxbits - l);
            while (total > (1u << maxbits)) {
                cnt[maxbits]--;
                for (int l = maxbits - 1; l > 0; l--)
                    if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
                total--;
            }
            int at = 0;
            for (int l = maxbits; l >= 1; l--)
                for (uint32_t k = 0; k < cnt[l] && at < m; k++) lens[W.ssym[at++]] = (uint8_t)l;
        }
    }
    L.sync();
}

// the canonical codes of lens[0 .. n), bit-reversed (lane 0)
template <class Lanes> INF_FN void dfl_codes(const Lanes& L, const uint8_t* lens, int n, uint16_t* codes)
{
    L.sync();
    if (L.lane() == 0) {
        uint32_t nextc[16], cnt[16];
        for (int l = 0; l < 16; l++) cnt[l] = 0;
        for (int s = 0; s < n; s++) cnt[lens[s] & 15]++;
        cnt[0] = 0;
        uint32_t c = 0;
        nextc[0] = 0;
        for (int l = 1; l < 16; l++) { c = (c + cnt[l - 1]) << 1; nextc[l] = c; }
        for (int s = 0; s < n; s++) {
            const int l = lens[s] & 15;
            uint32_t v = l ? nextc[l]++ : 0u, r = 0;
            for (int i = 0; i < l; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
            codes[s] = (uint16_t)r;
        }
    }
    L.sync();
}

INF_FN int dfl_cl_order(int i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? (19 - i) / 2 : 8 + (i - 4) / 2; }       // 16 17 18 0 8 7 9 6 10 5 ...

// the dynamic header: HLIT / HDIST trimmed, the lengths run-length coded into W.seq, the code-length code, HCLEN trimmed -> W.meta
template <class Lanes> INF_FN void dfl_header(const Lanes& L, DflWork& W)
{
    L.sync();
    if (L.lane() == 0) {
        int hlit = DFL_LL, hdist = DFL_D;
        while (hlit > 257 && W.len_ll[hlit - 1] == 0) hlit--;
        while (hdist > 1 && W.len_d[hdist - 1] == 0) hdist--;
        const int total = hlit + hdist;
        int ns = 0, i = 0;
        for (int s = 0; s < 20; s++) W.freq_cl[s] = 0;
#define DFL_AT(k) ((k) < hlit ? W.len_ll[(k)] : W.len_d[(k) - hlit])
#define DFL_EMIT(sym, x) do { if (ns < DFL_SEQ) W.seq[ns++] = (uint16_t)((sym) | ((x) << 8)); W.freq_cl[(sym)]++; } while (0)
        while (i < total) {
            const int v = DFL_AT(i);
            int run = 1;
            while (i + run < total && DFL_AT(i + run) == v) run++;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int k = run < 138 ? run : 138; DFL_EMIT(18, k - 11); run -= k; }
                if (run >= 3) { DFL_EMIT(17, run - 3); run = 0; }
                while (run-- > 0) DFL_EMIT(0, 0);
            } else {
                DFL_EMIT(v, 0); run--;
                while (run >= 3) { const int k = run < 6 ? run : 6; DFL_EMIT(16, k - 3); run -= k; }
                while (run-- > 0) DFL_EMIT(v, 0);
            }
        }
#undef DFL_AT
#undef DFL_EMIT
        W.meta[0] = (uint32_t)hlit; W.meta[1] = (uint32_t)hdist; W.meta[3] = (uint32_t)ns;
    }
    dfl_lengths(L, W, W.freq_cl, DFL_CL, 7, W.len_cl, true);
    dfl_codes(L, W.len_cl, DFL_CL, W.code_cl);
    if (L.lane() == 0) {
        int hclen = DFL_CL;
        while (hclen > 4 && W.len_cl[dfl_cl_order(hclen - 1)] == 0) hclen--;
        uint32_t bits = 14u + 3u * (uint32_t)hclen;
        const int ns = (int)W.meta[3];
        for (int k = 0; k < ns; k++) {
            const int s = W.seq[k] & 31;
            bits += W.len_cl[s < 20 ? s : 0] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
        }
        W.meta[2] = (uint32_t)hclen; W.meta[4] = bits;
    }
    L.sync();
}

// the bits of the codes in W for the tokens that were counted: literal/length and distance codes with their extra bits, and the end-of-block code
template <class Lanes> INF_FN uint32_t dfl_cost(const Lanes& L, const DflWork& W)
{
    uint32_t bits = 0;
#pragma GCC unroll 1
    for (int s = 0; s < DFL_LL; s++) bits += W.freq_ll[s] * (uint32_t)(W.len_ll[s] + (s > 256 ? inf_len_extra(s - 257) : 0));
#pragma GCC unroll 1
    for (int s = 0; s < DFL_D; s++) bits += W.freq_d[s] * (uint32_t)(W.len_d[s] + inf_dist_extra(s));
    return L.uni(bits);
}

template <class Lanes> INF_FN void dfl_fixed(const Lanes& L, DflWork& W)
{
    L.sync();
    for (int i = L.lane(); i < 288; i += L.width()) W.len_ll[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = L.lane(); i < 32; i += L.width()) W.len_d[i] = 5;
    L.sync();
}

// the code bits of a token, the first bit of the stream lowest; nb: how many (at most 15 + 5 + 15 + 13)
INF_FN uint64_t dfl_tok_bits(const DflWork& W, uint32_t t, int& nb)
{
    nb = 0;
    if (!(t & DFL_TOK)) return 0;
    if (!(t & DFL_TOK_MATCH)) { const int s = (int)(t & 255u); nb = W.len_ll[s]; return W.code_ll[s]; }
    int ls, lnx, lx, ds, dnx, dx;
    dfl_len_sym((int)((t >> 16) & 255u), ls, lnx, lx); dfl_dist_sym((int)(t & 0x7fffu), ds, dnx, dx);
    if (ls > 28) ls = 28;
    if (ds > DFL_D - 1) ds = DFL_D - 1;
    uint64_t v = W.code_ll[257 + ls];
    int k = W.len_ll[257 + ls];
    v |= (uint64_t)lx << k; k += lnx;
    v |= (uint64_t)W.code_d[ds] << k; k += W.len_d[ds];
    v |= (uint64_t)dx << k; k += dnx;
    nb = k;
    return v;
}

// ---- the writer: `acc` holds accn < 32 bits that wait for their word; wpos is that word's index in `out`.  Wave-uniform.
template <class Lanes> struct DflBits {
    uint8_t* out;
    uint64_t acc;
    int accn;
    int32_t wpos;
    Lanes L;
    INF_FN void word(int32_t w, uint32_t v) const
    {
        if (w >= 0 && w < DFL_SLOT / 4) { uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)}; memcpy(out + 4 * (size_t)w, b, 4); }
    }
    INF_FN void put(uint32_t v, int k)                             // k <= 16 bits, by every lane alike; lane 0 stores
    {
        acc |= (uint64_t)v << accn; accn += k;
        if (accn >= 32) {
            if (L.lane() == 0) word(wpos, (uint32_t)acc);
            acc >>= 32; accn -= 32; wpos++;
        }
    }
};

INF_FN void dfl_byte(uint8_t* out, int32_t at, uint32_t v) { if (at >= 0 && at < DFL_SLOT) out[at] = (uint8_t)v; }

// One BGZF block.  tok: n words of scratch; out: DFL_SLOT bytes, 4-byte aligned; crc_table: the 256 entries of inf_crc_entry;
// sizes (may be NULL): the payload bytes of the stored, the fixed and the dynamic coding of the same tokens.  Returns the block's
// size, or 0 when n is outside 0 .. DFL_MAX_IN (nothing written).
template <class Lanes> INF_FN int32_t dfl_block(const Lanes& L, DflWork& W, const uint8_t* in, int32_t n, uint32_t* tok, uint8_t* out, const uint32_t* crc_table, int32_t* sizes)
{
    if (n < 0 || n > DFL_MAX_IN) return 0;
    dfl_parse(L, W, in, n, tok);
    dfl_fixed(L, W);
    const uint32_t fixed_bytes = (3u + dfl_cost(L, W) + 7u) >> 3;
    dfl_lengths(L, W, W.freq_ll, 288, 15, W.len_ll, false);         // (286 and 287 never occur: their lengths are 0 again)
    dfl_lengths(L, W, W.freq_d, DFL_D, 15, W.len_d, false);
    if (L.lane() == 0) {                                           // a block without a match still declares one distance code
        int any = 0;
        for (int s = 0; s < DFL_D; s++) any |= W.len_d[s];
        if (!any) W.len_d[0] = 1;
    }
    dfl_header(L, W);
    const uint32_t dyn_bytes = (3u + L.uni(W.meta[4]) + dfl_cost(L, W) + 7u) >> 3, stored_bytes = 5u + (uint32_t)n;
    int mode = DFL_STORED;
    uint32_t best = stored_bytes;
    if (fixed_bytes < best) { mode = DFL_FIXED; best = fixed_bytes; }
    if (dyn_bytes < best) { mode = DFL_DYNAMIC; best = dyn_bytes; }
    if (sizes && L.lane() == 0) { sizes[0] = (int32_t)stored_bytes; sizes[1] = (int32_t)fixed_bytes; sizes[2] = (int32_t)dyn_bytes; }
    int32_t end = 18;                                              // the payload ends here
    if (mode == DFL_STORED) {
        if (L.lane() == 0) {
            dfl_byte(out, 18, 1u);
            dfl_byte(out, 19, (uint32_t)n & 255u); dfl_byte(out, 20, (uint32_t)n >> 8);
            dfl_byte(out, 21, ~(uint32_t)n & 255u); dfl_byte(out, 22, (~(uint32_t)n >> 8) & 255u);
        }
#pragma GCC unroll 1
        for (int32_t i = L.lane(); i < n; i += L.width()) dfl_byte(out, 23 + i, in[i]);
        end = 23 + n;
    } else {
        if (mode == DFL_FIXED) dfl_fixed(L, W);
        dfl_codes(L, W.len_ll, 288, W.code_ll);                     // (all 288: the fixed code's 9-bit codes start behind 286 and 287)
        dfl_codes(L, W.len_d, DFL_D, W.code_d);
        DflBits<Lanes> B{out, 0, 16, 4, L};                        // byte 18 = word 4, bit 16; bytes 16 and 17 (BSIZE) are written last
        B.put(1u, 1); B.put((uint32_t)mode, 2);
        if (mode == DFL_DYNAMIC) {
            const int hlit = (int)L.uni(W.meta[0]), hdist = (int)L.uni(W.meta[1]), hclen = (int)L.uni(W.meta[2]), ns = (int)L.uni(W.meta[3]);
            B.put((uint32_t)(hlit - 257), 5); B.put((uint32_t)(hdist - 1), 5); B.put((uint32_t)(hclen - 4), 4);
            for (int i = 0; i < hclen; i++) B.put(W.len_cl[dfl_cl_order(i)], 3);
#pragma GCC unroll 1
            for (int k = 0; k < ns && k < DFL_SEQ; k++) {
                const uint32_t e = L.uni(W.seq[k]);
                const int s = (int)(e & 31u) < 20 ? (int)(e & 31u) : 0;
                B.put(L.uni(W.code_cl[s]), (int)L.uni(W.len_cl[s]));
                if (s >= 16) B.put(e >> 8, s == 16 ? 2 : s == 17 ? 3 : 7);
            }
        }
        // the tokens, a tile at a time: bit counts, their prefix, the bits or-ed into the staging words, whole words to `out`
        for (int i = L.lane(); i < DFL_STAGE; i += L.width()) W.stage[i] = 0;
        L.sync();
#pragma GCC unroll 1
        for (int32_t b = 0; b < n; b += DFL_TILE) {
            for (int l = L.lane(); l < DFL_TILE; l += L.width()) {
                int nb = 0;
                if (b + l < n) (void)dfl_tok_bits(W, tok[b + l], nb);
                W.tnb[l] = (uint32_t)nb;
            }
            if (L.lane() == 0) W.stage[0] = (uint32_t)B.acc;
            L.sync();
            const uint32_t total = L.uni(L.scan64(W.tnb));
            L.sync();
            for (int l = L.lane(); l < DFL_TILE; l += L.width()) {
                int nb = 0;
                if (b + l >= n) continue;
                const uint64_t v = dfl_tok_bits(W, tok[b + l], nb);
                if (!nb) continue;
                const uint32_t off = (uint32_t)B.accn + W.tnb[l];
                const int w = (int)(off >> 5), sh = (int)(off & 31u);
                const uint64_t lo = v << sh;
                const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
                if ((uint32_t)lo && w < DFL_STAGE) L.or32(&W.stage[w], (uint32_t)lo);
                if ((uint32_t)(lo >> 32) && w + 1 < DFL_STAGE) L.or32(&W.stage[w + 1], (uint32_t)(lo >> 32));
                if (hi && w + 2 < DFL_STAGE) L.or32(&W.stage[w + 2], hi);
            }
            L.sync();
            const int full = (int)(((uint32_t)B.accn + total) >> 5);          // at most (31 + 64 * 48) / 32 = 96
            for (int i = L.lane(); i < full && i < DFL_STAGE; i += L.width()) B.word(B.wpos + i, W.stage[i]);
            const uint32_t carry = full < DFL_STAGE ? L.uni(W.stage[full]) : 0u;
            L.sync();
            for (int i = L.lane(); i <= full && i < DFL_STAGE; i += L.width()) W.stage[i] = 0;
            L.sync();
            B.acc = carry; B.accn = (int)(((uint32_t)B.accn + total) & 31u); B.wpos += full;
        }
        B.put(L.uni(W.code_ll[256]), (int)L.uni(W.len_ll[256]));
        const int tail = (B.accn + 7) >> 3;
        if (L.lane() == 0)
            for (int k = 0; k < tail; k++) dfl_byte(out, 4 * B.wpos + k, (uint32_t)(B.acc >> (8 * k)) & 255u);
        end = 4 * B.wpos + tail;
    }
    L.sync();
    const uint32_t crc = n > 0 ? L.crc(in, n, crc_table) : 0u;
    const int32_t size = end + 8;
    if (L.lane() == 0) {
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int k = 0; k < 16; k++) dfl_byte(out, k, head[k]);
        dfl_byte(out, 16, (uint32_t)(size - 1) & 255u); dfl_byte(out, 17, (uint32_t)(size - 1) >> 8);
        for (int k = 0; k < 4; k++) { dfl_byte(out, end + k, (crc >> (8 * k)) & 255u); dfl_byte(out, end + 4 + k, ((uint32_t)n >> (8 * k)) & 255u); }
    }
    L.sync();
    return size;
}

}  // namespace csv
