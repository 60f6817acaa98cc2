// sam_core.h — SAM text to BAM records, written once for the host and for the device.  Plain C++: no HIP
// header, no global state.  The rules live here, and nowhere else:
//   the line      one alignment line of SAM text (SAMv1 section 1.4) -> one BAM record (4.2), block_size included: sam_line_record,
//                 the serial form every host route uses and the judge of what the device's kernels (k_sam_*, at the end of bam.hip.h)
//                 write lane by lane.  The small rules both forms call: sam_base_code, sam_cigar_op, sam_int_type, sam_int_text,
//                 sam_float_class, sam_name_find, sam_bin.
//   the number    decimal text -> float32 is (float) strtod(text).  sam_float_text computes it without strtod when the text is
//                 [-+]?digits[.digits]?([eE][-+]?digits)? with at most 15 significant digits, at most 4 exponent digits and a decimal
//                 exponent of magnitude 22 or less (Clinger's fast path: the digits and the power of ten are exact doubles, one
//                 correctly rounded operation joins them).  Every other text is "slow": the host asks strtod, the device leaves a patch row.
//   the refusal   sam_refusal_text: what a refused line is told, behind "line <1-based number>: "; the same on every route.
//   the header    sam_header_parse (host only): the leading @ lines -> text, reference list, the name table sorted by bytes.
//   the windows   sam_window_end: where a window of text ends - behind the last line break inside window_bytes, or behind the first
//                 one after it when a line is longer.  The file written never depends on it.
// bin, the CG:B:I form of a long CIGAR and the 0xff qualities restate htslib's conventions from memory; the tests judge them against an
// independent writer from the specification, never against a file htslib made.
// tests/sam_core_main.cpp runs all of it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "index_core.h"

#if defined(__HIPCC__)
#define SAM_FN __host__ __device__ inline
#else
#define SAM_FN inline
#endif

namespace csv {

typedef long long sm_i64;
typedef unsigned long long sm_u64;

constexpr sm_i64 SAM_BLOCK = 65280;                   // bytes of the BAM stream per BGZF block (bgzip's cut, deflate_core.h's DFL_MAX_IN)
constexpr sm_i64 SAM_WINDOW = 64ll << 20;             // bytes of text per window when the caller names none
constexpr sm_i64 SAM_WINDOW_MAX = (1ll << 31) - 1;    // a window, and so a line, never has more
constexpr int SAM_MAX_OPS = 65535;                    // CIGAR operations n_cigar_op can say; more take the CG form
constexpr int SAM_NUM_MAX = 64;                       // bytes of the longest decimal text the number rules read (a wavefront's lanes)
constexpr int SAM_QNAME_MAX = 254;

enum {
    SAM_OK = 0, SAM_E_FIELDS, SAM_E_EMPTY_FIELD, SAM_E_EMPTY_LINE, SAM_E_CR, SAM_E_HEADER, SAM_E_QNAME, SAM_E_NUMBER, SAM_E_RANGE, SAM_E_RNAME, SAM_E_CIGAR,
    SAM_E_QUAL_LEN, SAM_E_QUAL_BYTE, SAM_E_TAG, SAM_E_TAG_RANGE, SAM_E_SIZE
};

SAM_FN sm_u64 sam_pow10(int k)                          // 0 <= k <= 18
{
    sm_u64 v = 1;
    for (int i = 0; i < k; i++) v *= 10;
    return v;
}

// 10^k, 0 <= k <= 22: exact in double
SAM_FN double sam_pow10d(int k)
{
    double v = 1.0;
    for (int i = 0; i < k; i++) v *= 10.0;               // (every partial product is an integer below 2^77 with at most 22 factors of 5: exact)
    return v;
}

// the 4-bit code of a base: the table =ACMGRSVTWYHKDBN without regard to case, 15 for every other byte
SAM_FN uint32_t sam_base_code(uint32_t c)
{
    if (c == '=') return 0;
    const uint32_t i = (c & 0xdfu) - 'A';
    if (i >= 26 || (c & 0xc0u) != 0x40u) return 15;
    return i < 16 ? (uint32_t)(0xFFF3FCFFB4FFD2E1ull >> (4 * i)) & 15u : (uint32_t)(0xFAF97F865Full >> (4 * (i - 16))) & 15u;
}

// MIDNSHP=X -> 0 .. 8, -1 for every other byte
SAM_FN int sam_cigar_op(uint32_t c)
{
    switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
    default: return -1;
    }
}
SAM_FN bool sam_op_on_ref(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
SAM_FN bool sam_digit(uint32_t c) { return c - '0' < 10u; }

// the type an i value takes, the smallest of c C s S i I that holds it (0: outside -2^31 .. 2^32 - 1), and its bytes
SAM_FN int sam_int_type(sm_i64 v, int* width)
{
    if (v < 0) {
        if (v >= -128) { *width = 1; return 'c'; }
        if (v >= -32768) { *width = 2; return 's'; }
        if (v >= -2147483648ll) { *width = 4; return 'i'; }
        *width = 0; return 0;
    }
    if (v <= 255) { *width = 1; return 'C'; }
    if (v <= 65535) { *width = 2; return 'S'; }
    if (v <= 4294967295ll) { *width = 4; return 'I'; }
    *width = 0; return 0;
}

// the width of a B subtype and the range of its integers (width 0: no subtype)
SAM_FN int sam_sub_width(uint32_t sub, sm_i64* lo, sm_i64* hi)
{
    switch (sub) {
    case 'c': *lo = -128; *hi = 127; return 1;
    case 'C': *lo = 0; *hi = 255; return 1;
    case 's': *lo = -32768; *hi = 32767; return 2;
    case 'S': *lo = 0; *hi = 65535; return 2;
    case 'i': *lo = -2147483648ll; *hi = 2147483647ll; return 4;
    case 'I': *lo = 0; *hi = 4294967295ll; return 4;
    case 'f': *lo = 0; *hi = 0; return 4;
    default: *lo = 0; *hi = 0; return 0;
    }
}

// [-+]?digits (the sign only where sign_ok) with at most 18 digits -> the value
SAM_FN bool sam_int_text(const uint8_t* p, sm_i64 n, bool sign_ok, sm_i64* v)
{
    sm_i64 i = 0;
    bool neg = false;
    if (n > 0 && sign_ok && (p[0] == '-' || p[0] == '+')) { neg = p[0] == '-'; i = 1; }
    if (n - i < 1 || n - i > 18) return false;
    sm_u64 a = 0;
    for (; i < n; i++) {
        if (!sam_digit(p[i])) return false;
        a = a * 10 + (p[i] - '0');
    }
    *v = neg ? -(sm_i64)a : (sm_i64)a;
    return true;
}

// what the grammar found in a float's text
struct SamFloat { int neg; sm_u64 mant; int nsig, nexp; sm_i64 exp10; };       // nsig: digits from the first non-zero one; nexp: exponent digits; exp10: exponent - fraction digits

// 2: the fast path, *f is (float) strtod(text); 1: slow
SAM_FN int sam_float_class(const SamFloat& q, float* f)
{
    if (q.nsig > 15 || q.nexp > 4 || q.exp10 > 22 || q.exp10 < -22) return 1;
    const double m = (double)q.mant;
    const double d = q.exp10 >= 0 ? m * sam_pow10d((int)q.exp10) : m / sam_pow10d((int)-q.exp10);
    *f = (float)(q.neg ? -d : d);
    return 2;
}

// the serial form of the grammar.  0: not the grammar (or more than SAM_NUM_MAX bytes); else sam_float_class's answer
SAM_FN int sam_float_text(const uint8_t* p, sm_i64 n, float* f)
{
    if (n < 1 || n > SAM_NUM_MAX) return 0;
    SamFloat q{0, 0, 0, 0, 0};
    sm_i64 i = 0;
    if (p[0] == '-' || p[0] == '+') { q.neg = p[0] == '-'; i = 1; }
    sm_i64 nd = 0, nfrac = 0;
    for (; i < n && sam_digit(p[i]); i++, nd++)
        if (q.nsig > 0 || p[i] != '0') { if (q.nsig < 15) q.mant = q.mant * 10 + (p[i] - '0'); q.nsig++; }
    if (nd == 0) return 0;
    if (i < n && p[i] == '.') {
        i++;
        for (; i < n && sam_digit(p[i]); i++, nfrac++)
            if (q.nsig > 0 || p[i] != '0') { if (q.nsig < 15) q.mant = q.mant * 10 + (p[i] - '0'); q.nsig++; }
        if (nfrac == 0) return 0;
    }
    sm_i64 e = 0;
    if (i < n && (p[i] == 'e' || p[i] == 'E')) {
        i++;
        bool eneg = false;
        if (i < n && (p[i] == '-' || p[i] == '+')) { eneg = p[i] == '-'; i++; }
        for (; i < n && sam_digit(p[i]); i++, q.nexp++)
            if (q.nexp < 4) e = e * 10 + (p[i] - '0');
        if (q.nexp == 0) return 0;
        if (eneg) e = -e;
    }
    if (i != n) return 0;
    q.exp10 = e - nfrac;
    return sam_float_class(q, f);
}

// the reference names sorted by their bytes (a name that is a prefix of another first), the ids beside them
struct SamNames { const uint8_t* blob; const int32_t* off; const int32_t* id; int32_t n; };          // off: n + 1

SAM_FN int sam_name_cmp(const uint8_t* a, sm_i64 na, const uint8_t* b, sm_i64 nb)
{
    const sm_i64 m = na < nb ? na : nb;
    for (sm_i64 i = 0; i < m; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : na > nb ? 1 : 0;
}

// the id of the name q[0 .. n), -2 when the header lacks it
SAM_FN int32_t sam_name_find(const SamNames& N, const uint8_t* q, sm_i64 n)
{
    int32_t lo = 0, hi = N.n - 1;
    while (lo <= hi) {
        const int32_t m = lo + (hi - lo) / 2;
        const int c = sam_name_cmp(q, n, N.blob + N.off[m], N.off[m + 1] - N.off[m]);
        if (c == 0) return N.id[m];
        if (c < 0) hi = m - 1; else lo = m + 1;
    }
    return -2;
}

// bin of a record at pos (-1: POS 0) over ref_len reference bases: reg2bin(pos, pos + max(ref_len, 1)), the low 16 bits
SAM_FN uint32_t sam_bin(sm_i64 pos, sm_i64 ref_len) { return ix_reg2bin(pos, pos + (ref_len > 1 ? ref_len : 1)) & 0xffffu; }

SAM_FN void sam_put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
SAM_FN void sam_put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
SAM_FN uint32_t sam_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the 32 fixed bytes behind block_size
struct SamFixed { int32_t refid, pos; uint32_t l_name, mapq, bin, n_cigar, flag, l_seq; int32_t next_refid, next_pos, tlen; };
SAM_FN void sam_put_fixed(uint8_t* p, const SamFixed& x)
{
    sam_put32(p, (uint32_t)x.refid); sam_put32(p + 4, (uint32_t)x.pos);
    p[8] = (uint8_t)x.l_name; p[9] = (uint8_t)x.mapq; sam_put16(p + 10, x.bin); sam_put16(p + 12, x.n_cigar); sam_put16(p + 14, x.flag);
    sam_put32(p + 16, x.l_seq); sam_put32(p + 20, (uint32_t)x.next_refid); sam_put32(p + 24, (uint32_t)x.next_pos); sam_put32(p + 28, (uint32_t)x.tlen);
}

// where a window that begins at w0 ends (exclusive; a line break is its last byte unless the text ends without one)
SAM_FN sm_i64 sam_window_end(const uint8_t* t, sm_i64 n, sm_i64 w0, sm_i64 window_bytes)
{
    if (n - w0 <= window_bytes) return n;
    sm_i64 e = w0 + window_bytes;
    while (e > w0 && t[e - 1] != '\n') e--;
    if (e > w0) return e;
    for (e = w0 + window_bytes; e < n && t[e] != '\n'; e++) {}
    return e < n ? e + 1 : n;
}

}  // namespace csv

#include <stdlib.h>

#include <string>
#include <vector>

namespace csv {

inline const char* sam_refusal_text(int why)
{
    switch (why) {
    case SAM_E_FIELDS: return "has fewer than 11 fields";
    case SAM_E_EMPTY_FIELD: return "has an empty field";
    case SAM_E_EMPTY_LINE: return "is empty";
    case SAM_E_CR: return "ends in a carriage return";
    case SAM_E_HEADER: return "is a header line behind the first alignment line";
    case SAM_E_QNAME: return "has a QNAME of more than 254 bytes";
    case SAM_E_NUMBER: return "has a field that is no decimal number";
    case SAM_E_RANGE: return "has a number outside its field's range";
    case SAM_E_RNAME: return "names a reference the header lacks";
    case SAM_E_CIGAR: return "has a bad CIGAR";
    case SAM_E_QUAL_LEN: return "has a QUAL whose length is not SEQ's";
    case SAM_E_QUAL_BYTE: return "has a QUAL byte below 33";
    case SAM_E_TAG: return "has an optional field that is not TAG:TYPE:VALUE";
    case SAM_E_TAG_RANGE: return "has a tag value outside its type";
    case SAM_E_SIZE: return "gives a record of 2^31 bytes or more";
    default: return "is refused";
    }
}

struct SamCounts { sm_i64 patches = 0, cg = 0; };

// One optional field t[b, e) appended to `out` as a BAM tag.  Slow floats are computed with strtod here (and counted): the host has
// no patch rows
inline int sam_tag_record(const uint8_t* t, sm_i64 b, sm_i64 e, std::vector<uint8_t>* out, SamCounts* cnt)
{
    const sm_i64 n = e - b;
    if (n < 5 || t[b + 2] != ':' || t[b + 4] != ':') return SAM_E_TAG;
    const uint8_t type = t[b + 3];
    const uint8_t* v = t + b + 5;
    const sm_i64 vn = n - 5;
    auto flt = [&](const uint8_t* p, sm_i64 k, uint8_t* dst) -> int {
        float f = 0;
        const int cls = sam_float_text(p, k, &f);
        if (cls != 2) {
            if (k < 1) return SAM_E_NUMBER;
            const std::string s((const char*)p, (size_t)k);
            if (s[0] == ' ' || s[0] == '\t' || s.find('\0') != std::string::npos) return SAM_E_NUMBER;
            char* end = nullptr;
            const double d = strtod(s.c_str(), &end);
            if (end != s.c_str() + s.size()) return SAM_E_NUMBER;
            f = (float)d;
            cnt->patches++;
        }
        sam_put32(dst, sam_float_bits(f));
        return SAM_OK;
    };
    out->push_back(t[b]); out->push_back(t[b + 1]);
    switch (type) {
    case 'A':
        if (vn != 1) return SAM_E_TAG;
        out->push_back('A'); out->push_back(v[0]);
        return SAM_OK;
    case 'i': {
        sm_i64 x;
        if (!sam_int_text(v, vn, true, &x)) return SAM_E_NUMBER;
        int w;
        const int ty = sam_int_type(x, &w);
        if (!ty) return SAM_E_TAG_RANGE;
        out->push_back((uint8_t)ty);
        for (int k = 0; k < w; k++) out->push_back((uint8_t)((sm_u64)x >> (8 * k)));
        return SAM_OK;
    }
    case 'f': {
        uint8_t q[4];
        const int rc = flt(v, vn, q);
        if (rc) return rc;
        out->push_back('f'); out->insert(out->end(), q, q + 4);
        return SAM_OK;
    }
    case 'H':
        if (vn & 1) return SAM_E_TAG;
        for (sm_i64 k = 0; k < vn; k++)
            if (!(sam_digit(v[k]) || (v[k] >= 'A' && v[k] <= 'F') || (v[k] >= 'a' && v[k] <= 'f'))) return SAM_E_TAG;
        /* fall through */
    case 'Z':
        out->push_back(type); out->insert(out->end(), v, v + vn); out->push_back(0);
        return SAM_OK;
    case 'B': {
        if (vn < 1 || (vn > 1 && v[1] != ',')) return SAM_E_TAG;
        sm_i64 lo, hi;
        const int w = sam_sub_width(v[0], &lo, &hi);
        if (!w) return SAM_E_TAG;
        out->push_back('B'); out->push_back(v[0]);
        const size_t at = out->size();
        out->insert(out->end(), 4, 0);
        uint32_t count = 0;
        for (sm_i64 p = 1; p < vn;) {                    // (p stands on a comma)
            sm_i64 q = p + 1;
            while (q < vn && v[q] != ',') q++;
            if (v[0] == 'f') {
                uint8_t b4[4];
                const int rc = flt(v + p + 1, q - p - 1, b4);
                if (rc) return rc;
                out->insert(out->end(), b4, b4 + 4);
            } else {
                sm_i64 x;
                if (!sam_int_text(v + p + 1, q - p - 1, true, &x)) return SAM_E_NUMBER;
                if (x < lo || x > hi) return SAM_E_TAG_RANGE;
                for (int k = 0; k < w; k++) out->push_back((uint8_t)((sm_u64)x >> (8 * k)));
            }
            count++;
            p = q;
        }
        sam_put32(out->data() + at, count);
        return SAM_OK;
    }
    default: return SAM_E_TAG;
    }
}

// The line rule, serial: the alignment line t[beg, end) (no line break inside) appended to `out` as one BAM record.  SAM_OK, or why
// the line is refused (`out` is then as it was)
inline int sam_line_record(const uint8_t* t, sm_i64 beg, sm_i64 end, const SamNames& N, std::vector<uint8_t>* out, SamCounts* cnt)
{
    if (end <= beg) return SAM_E_EMPTY_LINE;
    if (t[end - 1] == '\r') return SAM_E_CR;
    if (t[beg] == '@') return SAM_E_HEADER;
    std::vector<sm_i64> fb, fe;                          // the fields
    sm_i64 a = beg;
    bool empty = false;
    for (sm_i64 i = beg; i <= end; i++)
        if (i == end || t[i] == '\t') { fb.push_back(a); fe.push_back(i); if (i == a) empty = true; a = i + 1; }
    if (fb.size() < 11) return SAM_E_FIELDS;
    if (empty) return SAM_E_EMPTY_FIELD;
    const size_t base = out->size();
    struct Undo { std::vector<uint8_t>* o; size_t n; bool keep; ~Undo() { if (!keep) o->resize(n); } } undo{out, base, false};
    SamFixed x{};
    const sm_i64 l_name = fe[0] - fb[0];
    if (l_name > SAM_QNAME_MAX) return SAM_E_QNAME;
    x.l_name = (uint32_t)l_name + 1;
    sm_i64 v[9] = {0};
    const sm_i64 hi[9] = {0, 65535, 0, 2147483647, 255, 0, 0, 2147483647, 2147483647};
    for (int k : {1, 3, 4, 7, 8}) {
        if (!sam_int_text(t + fb[k], fe[k] - fb[k], k == 8, &v[k])) return SAM_E_NUMBER;
        if (v[k] > hi[k] || v[k] < -hi[k]) return SAM_E_RANGE;
    }
    x.flag = (uint32_t)v[1]; x.pos = (int32_t)(v[3] - 1); x.mapq = (uint32_t)v[4]; x.next_pos = (int32_t)(v[7] - 1); x.tlen = (int32_t)v[8];
    auto star = [&](int k) { return fe[k] - fb[k] == 1 && t[fb[k]] == '*'; };
    x.refid = star(2) ? -1 : sam_name_find(N, t + fb[2], fe[2] - fb[2]);
    if (x.refid == -2) return SAM_E_RNAME;
    if (star(6)) x.next_refid = -1;
    else if (fe[6] - fb[6] == 1 && t[fb[6]] == '=') x.next_refid = x.refid;
    else if ((x.next_refid = sam_name_find(N, t + fb[6], fe[6] - fb[6])) == -2) return SAM_E_RNAME;
    // CIGAR
    std::vector<uint32_t> ops;
    sm_i64 ref_len = 0;
    if (!star(5)) {
        sm_i64 len = 0, nd = 0;
        for (sm_i64 i = fb[5]; i < fe[5]; i++) {
            if (sam_digit(t[i])) { if (++nd > 9) return SAM_E_CIGAR; len = len * 10 + (t[i] - '0'); continue; }
            const int op = sam_cigar_op(t[i]);
            if (op < 0 || nd == 0 || len >= (1ll << 28)) return SAM_E_CIGAR;
            ops.push_back((uint32_t)len << 4 | (uint32_t)op);
            if (sam_op_on_ref(op)) ref_len += len;
            len = 0; nd = 0;
        }
        if (nd) return SAM_E_CIGAR;
    }
    const sm_i64 l_seq = star(9) ? 0 : fe[9] - fb[9];
    x.l_seq = (uint32_t)l_seq;
    const bool qstar = star(10);
    if (!qstar && fe[10] - fb[10] != l_seq) return SAM_E_QUAL_LEN;
    const bool cg = ops.size() > (size_t)SAM_MAX_OPS;
    x.n_cigar = cg ? 2 : (uint32_t)ops.size();
    x.bin = sam_bin(x.pos, ref_len);
    out->insert(out->end(), 36, 0);
    sam_put_fixed(out->data() + base + 4, x);
    out->insert(out->end(), t + fb[0], t + fe[0]); out->push_back(0);
    auto put_ops = [&](const uint32_t* p, size_t n) { for (size_t k = 0; k < n; k++) for (int s = 0; s < 32; s += 8) out->push_back((uint8_t)(p[k] >> s)); };
    if (cg) { const uint32_t two[2] = {(uint32_t)l_seq << 4 | 4u, (uint32_t)ref_len << 4 | 3u}; put_ops(two, 2); }
    else put_ops(ops.data(), ops.size());
    for (sm_i64 i = 0; i < l_seq; i += 2)
        out->push_back((uint8_t)(sam_base_code(t[fb[9] + i]) << 4 | (i + 1 < l_seq ? sam_base_code(t[fb[9] + i + 1]) : 0u)));
    for (sm_i64 i = 0; i < l_seq; i++) {
        if (qstar) { out->push_back(0xff); continue; }
        if (t[fb[10] + i] < 33) return SAM_E_QUAL_BYTE;
        out->push_back((uint8_t)(t[fb[10] + i] - 33));
    }
    for (size_t k = 11; k < fb.size(); k++) {
        const int rc = sam_tag_record(t, fb[k], fe[k], out, cnt);
        if (rc) return rc;
    }
    if (cg) {
        const uint8_t h[4] = {'C', 'G', 'B', 'I'};
        out->insert(out->end(), h, h + 4);
        for (int s = 0; s < 32; s += 8) out->push_back((uint8_t)((uint32_t)ops.size() >> s));
        put_ops(ops.data(), ops.size());
        cnt->cg++;
    }
    const size_t size = out->size() - base;
    if (size - 4 > 2147483647u) return SAM_E_SIZE;
    sam_put32(out->data() + base, (uint32_t)(size - 4));
    undo.keep = true;
    return SAM_OK;
}

// The header rule.  The leading @ lines of t[0, n) are the text, verbatim; the @SQ lines give the references in order.
struct SamHeader {
    sm_i64 text_bytes = 0, lines = 0;                    // the header's bytes (the first alignment line begins behind them) and lines
    std::vector<std::string> names;
    std::vector<sm_i64> lens;
    std::vector<uint8_t> image;                          // the BAM header: magic, l_text, text, n_ref, the reference list
    std::vector<uint8_t> blob;                           // the names sorted by bytes: SamNames over these three
    std::vector<int32_t> off, id;
    SamNames table() const { return SamNames{blob.data(), off.data(), id.data(), (int32_t)id.size()}; }
};

// false with a text: an @SQ line without SN or LN, an LN outside 1 .. 2^31 - 1, a name that appears twice, alignment lines without any @SQ
inline bool sam_header_parse(const uint8_t* t, sm_i64 n, SamHeader* H, std::string* err)
{
    *H = SamHeader();
    sm_i64 at = 0;
    while (at < n && t[at] == '@') {
        sm_i64 e = at;
        while (e < n && t[e] != '\n') e++;
        H->lines++;
        if (e - at >= 3 && t[at + 1] == 'S' && t[at + 2] == 'Q' && (e - at == 3 || t[at + 3] == '\t')) {
            std::string name;
            sm_i64 ln = -1;
            bool has_name = false;
            for (sm_i64 f = at + 3; f < e;) {                                // the fields: each begins behind a tab
                sm_i64 fe = f + 1;
                while (fe < e && t[fe] != '\t') fe++;
                sm_i64 ve = fe;
                if (ve > f + 1 && t[ve - 1] == '\r' && fe == e) ve--;
                if (ve - f - 1 >= 3 && t[f + 1] == 'S' && t[f + 2] == 'N' && t[f + 3] == ':' && !has_name) { name.assign((const char*)t + f + 4, (size_t)(ve - f - 4)); has_name = true; }
                if (ve - f - 1 >= 3 && t[f + 1] == 'L' && t[f + 2] == 'N' && t[f + 3] == ':' && ln < 0)
                    if (!sam_int_text(t + f + 4, ve - f - 4, false, &ln) || ln < 1 || ln > 2147483647) ln = -2;
                f = fe;
            }
            if (!has_name || name.empty() || ln < 0) {
                *err = "line " + std::to_string(H->lines) + ": an @SQ line needs SN and an LN of 1 .. 2147483647";
                return false;
            }
            H->names.push_back(name); H->lens.push_back(ln);
        }
        at = e < n ? e + 1 : n;
    }
    H->text_bytes = at;
    const size_t nr = H->names.size();
    if (at < n && nr == 0) { *err = "line " + std::to_string(H->lines + 1) + ": an alignment line, and the header has no @SQ line"; return false; }
    if ((sm_u64)at > 2147483647ull) { *err = "the header has 2^31 bytes or more"; return false; }
    std::vector<int32_t> order(nr);
    for (size_t i = 0; i < nr; i++) order[i] = (int32_t)i;
    struct Less { const std::vector<std::string>* v; bool operator()(int32_t a, int32_t b) const {
        return sam_name_cmp((const uint8_t*)(*v)[a].data(), (sm_i64)(*v)[a].size(), (const uint8_t*)(*v)[b].data(), (sm_i64)(*v)[b].size()) < 0; } } less{&H->names};
    // heap sort of the index list (no <algorithm> here)
    auto sift = [&](size_t root, size_t end) {
        while (2 * root + 1 < end) {
            size_t c = 2 * root + 1;
            if (c + 1 < end && less(order[c], order[c + 1])) c++;
            if (!less(order[root], order[c])) return;
            const int32_t tmp = order[root]; order[root] = order[c]; order[c] = tmp;
            root = c;
        }
    };
    for (size_t s = nr / 2; s-- > 0;) sift(s, nr);
    for (size_t e = nr; e-- > 1;) { const int32_t tmp = order[0]; order[0] = order[e]; order[e] = tmp; sift(0, e); }
    H->off.push_back(0);
    for (size_t k = 0; k < nr; k++) {
        const std::string& s = H->names[(size_t)order[k]];
        if (k && s == H->names[(size_t)order[k - 1]]) { *err = "the header names the reference " + s + " twice"; return false; }
        H->blob.insert(H->blob.end(), s.begin(), s.end());
        H->off.push_back((int32_t)H->blob.size());
        H->id.push_back(order[k]);
    }
    H->blob.insert(H->blob.end(), 64, 0);                 // (room for a wavefront's read of 64 bytes at the last name)
    std::vector<uint8_t>& im = H->image;
    const uint8_t magic[4] = {'B', 'A', 'M', 1};
    im.insert(im.end(), magic, magic + 4);
    uint8_t w[4];
    sam_put32(w, (uint32_t)at); im.insert(im.end(), w, w + 4);
    im.insert(im.end(), t, t + at);
    sam_put32(w, (uint32_t)nr); im.insert(im.end(), w, w + 4);
    for (size_t i = 0; i < nr; i++) {
        sam_put32(w, (uint32_t)H->names[i].size() + 1); im.insert(im.end(), w, w + 4);
        im.insert(im.end(), H->names[i].begin(), H->names[i].end()); im.push_back(0);
        sam_put32(w, (uint32_t)H->lens[i]); im.insert(im.end(), w, w + 4);
    }
    return true;
}

// the text of a refusal; line: 1-based in the file
inline std::string sam_refusal(sm_i64 line, int why) { return "line " + std::to_string(line) + " " + sam_refusal_text(why); }

// The lines of the window t[w0, w1) (whole lines; the last may lack its line break) from line ordinal first_line on (0-based in the file)
// -> their records appended to `out`.  SAM_OK, or the first refusal with its line in *bad_line (1-based)
inline int sam_window_records(const uint8_t* t, sm_i64 w0, sm_i64 w1, sm_i64 first_line, const SamNames& N, std::vector<uint8_t>* out, SamCounts* cnt, sm_i64* n_lines,
                              sm_i64* bad_line)
{
    sm_i64 line = first_line;
    for (sm_i64 a = w0; a < w1; line++) {
        const uint8_t* nl = (const uint8_t*)memchr(t + a, '\n', (size_t)(w1 - a));
        const sm_i64 e = nl ? nl - t : w1;
        const int why = sam_line_record(t, a, e, N, out, cnt);
        if (why) { *bad_line = line + 1; if (n_lines) *n_lines = line - first_line; return why; }
        a = e + 1;
    }
    if (n_lines) *n_lines = line - first_line;
    return SAM_OK;
}

// The SAM file as one read-only mapping (the windows are cuts of it; nothing is copied on the host route)
struct SamMap {
    const uint8_t* t = nullptr; sm_i64 n = 0;
    bool open(const char* path, std::string* err);
    void close();
    ~SamMap() { close(); }
};

}  // namespace csv

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace csv {

inline bool SamMap::open(const char* path, std::string* err)
{
    close();
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) { *err = std::string("cannot open ") + path; return false; }
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd); *err = std::string(path) + " is no regular file"; return false; }
    n = (sm_i64)st.st_size;
    if (n > 0) {
        void* p = mmap(nullptr, (size_t)n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) { ::close(fd); n = 0; *err = std::string("cannot map ") + path; return false; }
        t = (const uint8_t*)p;
    }
    ::close(fd);
    return true;
}
inline void SamMap::close()
{
    if (t) munmap((void*)t, (size_t)n);
    t = nullptr; n = 0;
}

// counts of csv_sam_stats, in its order
struct SamStats {
    sm_i64 lines = 0, records = 0, header_bytes = 0, text_bytes = 0, stream_bytes = 0, out_bytes = 0, blocks = 0, windows = 0, patches = 0, cg = 0, up = 0, down = 0;
    double ms[4] = {0, 0, 0, 0};                          // device time of lines / plan / write / deflate
};
constexpr int SAM_N_COUNTS = 12;
inline void sam_stats_out(const SamStats& s, int64_t* counts, double* ms)
{
    const sm_i64 v[SAM_N_COUNTS] = {s.lines, s.records, s.header_bytes, s.text_bytes, s.stream_bytes, s.out_bytes, s.blocks, s.windows, s.patches, s.cg, s.up, s.down};
    if (counts) for (int k = 0; k < SAM_N_COUNTS; k++) counts[k] = v[k];
    if (ms) for (int k = 0; k < 4; k++) ms[k] = s.ms[k];
}

static const uint8_t SAM_EOF_BLOCK[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace csv
