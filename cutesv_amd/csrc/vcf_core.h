// vcf_core.h — the text of one VCF record, written once for the host and for the device.  Plain C++: no HIP
// header, no global state.  The rules of generate_output (cuteSV_genotype.py:242-467) that decide WHAT a record holds live here and
// nowhere else:
//   * vcf_emitted_id    the size filters: is the call written, and under which SVID counter
//   * vcf_ref_range     the contig bases the record reads (csv_vcf_ref_ranges hands them out, both emitters read them)
//   * vcf_interval      the tabix interval of a record (the text parser of csv_tbx_build and the rows of the device emitter)
//   * vcf_af            str(round(dv / (dv + dr), 4)) without printf
// and vcf_record, the record of one call over a VcfView - the calls as flat columns plus the small tables (segments, chromosome
// names, strand strings, genotype strings) - written by the lanes of a VcfSink: one lane on the host (csv_vcf_emit_core_host, what
// the CPU tests and tests/vcf_core_main.cpp run), the 64 lanes of a wavefront on the device (k_vcf_write in vcf_strings.hip.h).  A
// sink without an output only counts: that is vcf_record_len.  csrc/vcf_emit.cpp's emit_slice stays the yardstick: vcf_record gives
// its bytes, and tests/test_vcf_core.py holds it to that.
//
// Bounds: vcf_record trusts its view.  vcf_host_prepare (vcf_emit.cpp) is the check that earns that trust, made on the host before
// anything runs: every segment, chromosome, strand and mate index lies inside its table, every genotyped call has a table row, every
// call's REF bytes are as many as its range.  With it every read is inside the call's own slice of a blob or inside a table entry,
// and a write goes to out[o .. o + vcf_record_len).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/cutesv_hip.h"

#if defined(__HIPCC__)
#define VCF_FN __host__ __device__ inline
#else
#define VCF_FN inline
#endif

namespace csv {

typedef long long vcf_i64;
typedef unsigned long long vcf_u64;

enum { VCF_ID_INS = 0, VCF_ID_DEL = 1, VCF_ID_BND = 2, VCF_ID_DUP = 3, VCF_ID_INV = 4 };      // svid[5] of csv_vcf_emit (main script :1209-1213)

// size filters of generate_output (cuteSV_genotype.py:265-268, 315-316, 351-352): is the call written, and under which counter
VCF_FN int vcf_emitted_id(int type, vcf_i64 bp1, vcf_i64 bp2, vcf_i64 min_size, vcf_i64 max_size)
{
    if (type == CSV_DEL || type == CSV_INS) {
        if ((bp2 > max_size && max_size != -1) || bp2 < min_size) return -1;
        return type == CSV_INS ? VCF_ID_INS : VCF_ID_DEL;
    }
    if (type == CSV_DUP || type == CSV_INV) {
        const vcf_i64 len = bp2 - bp1;
        if ((len < 0 ? -len : len) > max_size && max_size != -1) return -1;
        return type == CSV_DUP ? VCF_ID_DUP : VCF_ID_INV;
    }
    return VCF_ID_BND;
}

// The contig bases the record of a call reads: [b, e), of which a DEL record prints [b, slice_e) as its REF (generate_output: INS
// :297, DEL :299-300, DUP :334, INV :360-365, BND :431-434).  Empty (b == e): a call the size filters drop (id < 0), or INS / DEL
// under ignore_sequence.  inv_pp: the INV call's strand string is "++"; slen: the contig's length, 0 for a contig without sequence;
// a range that is not inside [0, slen) is the caller's to judge ('N' for BND, CSV_E_INVALID otherwise).
struct VcfRefRange { vcf_i64 b, e, slice_e; bool bnd; };
VCF_FN VcfRefRange vcf_ref_range(int id, int type, bool ignore_sequence, vcf_i64 pos, vcf_i64 bp2, int aux, bool inv_pp, vcf_i64 slen)
{
    VcfRefRange r{0, 0, 0, false};
    if (id < 0) return r;
    const vcf_i64 prev = pos - 1 > 0 ? pos - 1 : 0;
    if (type == CSV_DEL || type == CSV_INS) {
        if (ignore_sequence) return r;
        r.b = prev; r.e = r.slice_e = prev + 1;                                        // ref_chrom[max(pos-1, 0)] (:297)
        if (type == CSV_DEL) {
            vcf_i64 r1 = pos + bp2;                                                     // slice end, clamped like Python
            if (r1 > slen) r1 = slen;
            r.slice_e = r1 > prev ? r1 : prev;
            if (r1 > r.e) r.e = r1;
        }
    } else if (type == CSV_DUP) {
        r.b = pos; r.e = pos + 1;                                                       // ref_chrom[int(i[2])] (:334)
    } else if (type == CSV_INV) {
        r.b = inv_pp ? prev : pos; r.e = r.b + 1;                                       // :360-365
    } else {
        const bool nfirst = (aux & 7) < 2;                                              // ALT starts with 'N' (types A/B)
        r.b = nfirst ? prev : pos; r.e = r.b + 1; r.bnd = true;
    }
    return r;
}
VCF_FN bool vcf_range_inside(const VcfRefRange& r, vcf_i64 slen) { return r.b >= 0 && r.e <= slen; }

// The interval of a VCF data line, 0-based and half open - the one place the rule lives: beg = POS - 1; end = INFO's END when the
// line has one and it is greater than beg, else beg + len(REF).  It restates htslib's rule for VCF from memory.
VCF_FN void vcf_interval(vcf_i64 pos, vcf_i64 ref_len, bool has_end, vcf_i64 end_value, vcf_i64* beg, vcf_i64* end)
{
    *beg = pos - 1;
    *end = (has_end && end_value > *beg) ? end_value : *beg + ref_len;
}

// trans_table = str.maketrans('RYSWKMBDHV', 'ACCAGACAAA')   (cuteSV_genotype.py:262)
VCF_FN uint8_t vcf_iupac(uint8_t c)
{
    switch (c) {
    case 'R': return 'A'; case 'Y': return 'C'; case 'S': return 'C'; case 'W': return 'A'; case 'K': return 'G';
    case 'M': return 'A'; case 'B': return 'C'; case 'D': return 'A'; case 'H': return 'A'; case 'V': return 'A';
    default: return c;
    }
}

// ---------------------------------------------------------------------------------------- AF
// str(round(dv / (dv + dr), 4)) (cuteSV_genotype.py:284) as the host emitter prints it: "%.4f" of the IEEE double dv / (dv + dr),
// trailing zeros trimmed down to one decimal.  dv >= 0, dr >= 0, dv + dr > 0 (vcf_host_prepare refuses anything else), so the
// quotient q lies in [0, 1]: q = m * 2^-s with the integer m < 2^53 and s >= 52.  m * 10^4 < 2^67 is held exactly in 128 bits, its
// quotient by 2^s is the four-decimal value and the remainder says which way the tie-to-even rounding of printf goes - on the
// exact binary value, as glibc rounds.  The text comes back packed: byte k of `text` is character k, n of them (3 .. 6).
struct VcfAf { vcf_u64 text; int n; };
VCF_FN VcfAf vcf_af(vcf_i64 dv, vcf_i64 dr)
{
    const double q = (double)dv / (double)(dv + dr);                                    // one correctly rounded fp64 division
    vcf_u64 bits;
    memcpy(&bits, &q, 8);
    const int ex = (int)((bits >> 52) & 0x7ff);
    const vcf_u64 m = ex ? ((bits & ((1ull << 52) - 1)) | (1ull << 52)) : (bits & ((1ull << 52) - 1));
    const int s = ex ? 1075 - ex : 1074;
    unsigned n4 = 0;                                                                    // round_half_even(q * 10^4), 0 .. 10000
    if (s < 70) {                                                                       // (beyond: q * 10^4 < 2^-2, it rounds to 0)
        // m * 10^4 in two words: hi * 2^32 + lo with lo < 2^32
        const vcf_u64 p0 = (m & 0xffffffffull) * 10000ull, p1 = (m >> 32) * 10000ull + (p0 >> 32);
        const vcf_u64 lo = p0 & 0xffffffffull;                                           // value = p1 * 2^32 + lo, p1 < 2^35
        // quotient and remainder by 2^s, s in [52, 70): the value's bits from s up, and the bits below against 2^(s-1)
        vcf_u64 quo, rem_hi, rem_lo;                                                    // remainder = rem_hi * 2^32 + rem_lo
        if (s >= 67) { quo = 0; rem_hi = p1; rem_lo = lo; }
        else { quo = p1 >> (s - 32); rem_hi = p1 & ((1ull << (s - 32)) - 1); rem_lo = lo; }
        // half = 2^(s-1) = (2^(s-33)) * 2^32 (s >= 52: no low word)
        const vcf_u64 half_hi = 1ull << (s - 33);
        const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > 0), tie = rem_hi == half_hi && rem_lo == 0;
        n4 = (unsigned)quo + ((above || (tie && (quo & 1))) ? 1u : 0u);
    }
    const unsigned ip = n4 / 10000u, fr = n4 % 10000u;
    const int nd = fr % 10u ? 4 : fr % 100u ? 3 : fr % 1000u ? 2 : 1;                   // decimals kept (no array: nothing for scratch memory)
    VcfAf a{(vcf_u64)('0' + ip) | ((vcf_u64)'.' << 8), 2 + nd};
    a.text |= (vcf_u64)('0' + fr / 1000u) << 16 | (vcf_u64)('0' + (fr / 100u) % 10u) << 24 | (vcf_u64)('0' + (fr / 10u) % 10u) << 32 | (vcf_u64)('0' + fr % 10u) << 40;
    return a;
}

// ---------------------------------------------------------------------------------------- the view
// The calls as flat columns (one entry per call, in the call order of the batch), the per-call blobs (call c's bytes are
// blob[off[c] .. off[c + 1]); a NULL offset column: no call has any) and the small tables.  Every pointer is host memory for the host
// form and device memory for the kernels.  gl: the genotype strings of the keys that occur - gl_key ascending, row r's four strings
// (GT, PL, GQ, QUAL) are gl[gl_off[4 r + k] .. gl_off[4 r + k + 1]), gl_flag[r] bit 0: QUAL is a number below 5 (the q5 filter),
// bit 1: GT is "0/0" (IMPRECISE) - the two facts the host derives from the strings, so that no strtod runs on the device.
struct VcfView {
    vcf_i64 n_calls;
    const int32_t *call_seg, *call_aux, *support, *cipos, *cilen, *dr, *gl_idx;
    const vcf_i64 *bp1, *bp2;
    const vcf_i64* ref_off; const uint8_t* ref;
    const vcf_i64* alt_off; const uint8_t* alt;
    const vcf_i64* rn_off;  const uint8_t* rn;
    const int32_t *seg_type, *seg_chrom, *seg_gt;                   // per segment: svtype, chromosome, the `action` flag
    int32_t n_chrom;
    const int32_t* chrom_off; const uint8_t* chrom; const vcf_i64* chrom_len;       // names back to back, n_chrom + 1 offsets; lengths (0: no sequence)
    int32_t n_strand;
    const int32_t* strand_off; const uint8_t* strand;              // INV strand strings by call_aux code
    int32_t n_gl;
    const int32_t* gl_key; const int32_t* gl_off; const uint8_t* gl; const uint8_t* gl_flag;
    vcf_i64 min_size, max_size;
    int32_t genotype, report_readid, ignore_sequence;
};

VCF_FN int vcf_call_type(const VcfView& V, vcf_i64 c) { return V.seg_type[V.call_seg[c]]; }
VCF_FN int vcf_call_id(const VcfView& V, vcf_i64 c) { return vcf_emitted_id(vcf_call_type(V, c), V.bp1[c], V.bp2[c], V.min_size, V.max_size); }
VCF_FN bool vcf_strand_pp(const VcfView& V, int code)
{
    const int b = V.strand_off[code];
    return V.strand_off[code + 1] - b == 2 && V.strand[b] == '+' && V.strand[b + 1] == '+';
}
VCF_FN VcfRefRange vcf_call_range(const VcfView& V, vcf_i64 c, int id)
{
    const int type = vcf_call_type(V, c);
    const bool pp = type == CSV_INV && id >= 0 && vcf_strand_pp(V, V.call_aux[c]);
    return vcf_ref_range(id, type, V.ignore_sequence != 0, V.bp1[c], V.bp2[c], V.call_aux[c], pp, V.chrom_len[V.seg_chrom[V.call_seg[c]]]);
}
// row of key in gl_key, -1 when the table has none
VCF_FN int vcf_gl_row(const VcfView& V, int key)
{
    int lo = 0, hi = V.n_gl;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (V.gl_key[mid] < key) lo = mid + 1; else hi = mid; }
    return (lo < V.n_gl && V.gl_key[lo] == key) ? lo : -1;
}

// ---------------------------------------------------------------------------------------- the sink
// `width` lanes write a record together: every lane runs the same calls with the same arguments, lane l stores the bytes l, l + width,
// ... of each piece (neighbouring lanes store neighbouring bytes).  out == NULL: nothing is stored, o counts.
struct VcfSink { uint8_t* out; vcf_i64 o; int lane, width; };

VCF_FN void vcf_put(VcfSink& S, const uint8_t* src, vcf_i64 n)
{
    if (S.out) for (vcf_i64 x = S.lane; x < n; x += S.width) S.out[S.o + x] = src[x];
    S.o += n;
}
VCF_FN void vcf_put_mapped(VcfSink& S, const uint8_t* src, vcf_i64 n)                   // the IUPAC table on the way
{
    if (S.out) for (vcf_i64 x = S.lane; x < n; x += S.width) S.out[S.o + x] = vcf_iupac(src[x]);
    S.o += n;
}
template <int N> VCF_FN void vcf_lit(VcfSink& S, const char (&s)[N])
{
    if (S.out) for (int x = S.lane; x < N - 1; x += S.width) S.out[S.o + x] = (uint8_t)s[x];
    S.o += N - 1;
}
VCF_FN void vcf_ch(VcfSink& S, uint8_t c)
{
    if (S.out && S.lane == 0) S.out[S.o] = c;
    S.o += 1;
}
VCF_FN vcf_u64 vcf_pow10(int k)
{
    vcf_u64 p = 1;
    for (int i = 0; i < k; i++) p *= 10ull;
    return p;
}
// v in decimal, one lane per digit (a quotient by a power of ten each: no digit buffer)
VCF_FN void vcf_num(VcfSink& S, vcf_i64 v)
{
    const vcf_u64 u = v < 0 ? 0ull - (vcf_u64)v : (vcf_u64)v;
    if (v < 0) vcf_ch(S, '-');
    int nd = 1;                                                                         // u <= 2^63 < 10^19: at most 19 digits
    for (vcf_u64 p = 10; nd < 19 && u >= p; p *= 10ull) nd++;
    if (S.out) for (int x = S.lane; x < nd; x += S.width) S.out[S.o + x] = (uint8_t)('0' + (u / vcf_pow10(nd - 1 - x)) % 10ull);
    S.o += nd;
}
VCF_FN void vcf_packed(VcfSink& S, vcf_u64 text, int n)                                 // n <= 8 characters packed into a word
{
    if (S.out) for (int x = S.lane; x < n; x += S.width) S.out[S.o + x] = (uint8_t)(text >> (8 * x));
    S.o += n;
}

// ---------------------------------------------------------------------------------------- the record
// What the record of call c says about itself beside its text: written at all, its chromosome, and its tabix interval
struct VcfRow { vcf_i64 beg, end; int chrom; };

// The record of call c as emit_slice writes it, byte for byte; svid: the number its ID carries.  The caller has made sure the call is
// emitted (id = vcf_call_id(V, c) >= 0).  row (nullable) receives the chromosome and the interval of the record.
VCF_FN void vcf_record(const VcfView& V, vcf_i64 c, int id, vcf_i64 svid, VcfSink& S, VcfRow* row)
{
    const int sg = V.call_seg[c], type = V.seg_type[sg], ch = V.seg_chrom[sg], aux = V.call_aux[c];
    // TRA calls whose count_coverage gave up carry the '.' fields too (cuteSV_resolveTRA.py:276-281)
    const int gr = (V.seg_gt[sg] != 0 && V.gl_idx[c] >= 0) ? vcf_gl_row(V, V.gl_idx[c]) : -1;
    const bool gt_on = gr >= 0;
    const int flag = gt_on ? V.gl_flag[gr] : 0;
    const vcf_i64 pos = V.bp1[c], re = V.support[c];
    const VcfRefRange rr = vcf_call_range(V, c, id);
    const uint8_t* mine = V.ref + V.ref_off[c];
    const bool readable = V.ref_off[c + 1] > V.ref_off[c];
    const uint8_t* cname = V.chrom + V.chrom_off[ch];
    const int cname_n = V.chrom_off[ch + 1] - V.chrom_off[ch];
    auto gl_field = [&](int k) { vcf_put(S, V.gl + V.gl_off[4 * gr + k], V.gl_off[4 * gr + k + 1] - V.gl_off[4 * gr + k]); };
    auto qual_filter_precise = [&]() {                     // \t QUAL \t FILTER \t PRECISE|IMPRECISE
        vcf_ch(S, '\t');
        if (gt_on) gl_field(3); else vcf_ch(S, '.');
        if (flag & 1) vcf_lit(S, "\tq5\t"); else vcf_lit(S, "\tPASS\t");
        if (flag & 2) vcf_lit(S, "IMPRECISE"); else vcf_lit(S, "PRECISE");
    };
    auto rnames = [&]() {
        if (!V.report_readid) return;
        vcf_lit(S, ";RNAMES=");
        if (V.rn_off) vcf_put(S, V.rn + V.rn_off[c], V.rn_off[c + 1] - V.rn_off[c]);
    };
    auto af = [&]() {
        if (!V.genotype) return;
        vcf_lit(S, ";AF=");
        if (gt_on) { const VcfAf a = vcf_af(re, V.dr[c]); vcf_packed(S, a.text, a.n); } else vcf_ch(S, '.');
    };
    auto tail = [&]() {                                    // FORMAT + sample
        vcf_lit(S, "\tGT:DR:DV:PL:GQ\t");
        if (gt_on) gl_field(0); else vcf_lit(S, "./.");
        vcf_ch(S, ':');
        if (gt_on) vcf_num(S, V.dr[c]); else vcf_ch(S, '.');
        vcf_ch(S, ':'); vcf_num(S, re); vcf_ch(S, ':');
        if (gt_on) gl_field(1); else vcf_lit(S, ".,.,.");
        vcf_ch(S, ':');
        if (gt_on) gl_field(2); else vcf_ch(S, '.');
        vcf_ch(S, '\n');
    };
    vcf_i64 vpos, ref_len = 1, end_value = 0;
    bool has_end = true;
    vcf_put(S, cname, cname_n); vcf_ch(S, '\t');
    if (type == CSV_DEL || type == CSV_INS) {
        const vcf_i64 len = V.bp2[c];                                                   // |SVLEN|
        end_value = type == CSV_INS ? pos : pos + len;
        vpos = pos;
        vcf_num(S, pos);
        if (type == CSV_INS) vcf_lit(S, "\tcuteSV.INS."); else vcf_lit(S, "\tcuteSV.DEL.");
        vcf_num(S, svid); vcf_ch(S, '\t');
        if (V.ignore_sequence) {
            if (type == CSV_INS) vcf_lit(S, "N\t<INS>"); else vcf_lit(S, "N\t<DEL>");
        } else if (type == CSV_INS) {
            vcf_ch(S, vcf_iupac(mine[0])); vcf_ch(S, '\t'); vcf_ch(S, mine[0]);        // ref_chrom[max(pos-1, 0)] (:297)
            if (V.alt_off) vcf_put(S, V.alt + V.alt_off[c], V.alt_off[c + 1] - V.alt_off[c]);
        } else {
            ref_len = rr.slice_e - rr.b;
            vcf_put_mapped(S, mine, ref_len);                                           // the deleted bases
            vcf_ch(S, '\t'); vcf_ch(S, mine[0]);
        }
        qual_filter_precise();
        if (type == CSV_INS) vcf_lit(S, ";SVTYPE=INS;SVLEN="); else vcf_lit(S, ";SVTYPE=DEL;SVLEN=");
        vcf_num(S, type == CSV_INS ? len : -len);
        vcf_lit(S, ";END="); vcf_num(S, end_value);
        vcf_lit(S, ";CIPOS=-"); vcf_num(S, V.cipos[c]); vcf_ch(S, ','); vcf_num(S, V.cipos[c]);
        vcf_lit(S, ";CILEN=-"); vcf_num(S, V.cilen[c]); vcf_ch(S, ','); vcf_num(S, V.cilen[c]);
        vcf_lit(S, ";RE="); vcf_num(S, re);
        rnames();
        af();
        if (type == CSV_DEL) vcf_lit(S, ";STRAND=+-");
    } else if (type == CSV_DUP || type == CSV_INV) {
        const vcf_i64 len = V.bp2[c] - V.bp1[c], alen = len < 0 ? -len : len;
        const bool pp = type == CSV_INV && vcf_strand_pp(V, aux);                       // :360-365
        vpos = (type == CSV_DUP || !pp) ? pos + 1 : pos;
        end_value = vpos + alen;
        vcf_num(S, vpos);
        if (type == CSV_DUP) vcf_lit(S, "\tcuteSV.DUP."); else vcf_lit(S, "\tcuteSV.INV.");
        vcf_num(S, svid); vcf_ch(S, '\t');
        vcf_ch(S, vcf_iupac(mine[0]));
        if (type == CSV_DUP) vcf_lit(S, "\t<DUP>"); else vcf_lit(S, "\t<INV>");
        qual_filter_precise();
        if (type == CSV_DUP) vcf_lit(S, ";SVTYPE=DUP;SVLEN="); else vcf_lit(S, ";SVTYPE=INV;SVLEN=");
        vcf_num(S, len);
        vcf_lit(S, ";END="); vcf_num(S, end_value);
        vcf_lit(S, ";RE="); vcf_num(S, re);
        if (type == CSV_DUP) vcf_lit(S, ";STRAND=-+");
        else { vcf_lit(S, ";STRAND="); vcf_put(S, V.strand + V.strand_off[aux], V.strand_off[aux + 1] - V.strand_off[aux]); }
        rnames();
        af();
    } else {                                                                            // BND (:400-458)
        const int code = aux & 7, c2 = aux >> 3;
        const vcf_i64 mate = V.bp2[c] + ((code == 0 || code == 2) ? 1 : 0);             // TRA:140
        const uint8_t b0 = readable ? mine[0] : (uint8_t)'N';                           // try/except -> 'N' (:431-434)
        const uint8_t br = (code == 0 || code == 2) ? '[' : ']';
        has_end = false;
        vpos = code < 2 ? pos : pos + 1;
        vcf_num(S, vpos);
        vcf_lit(S, "\tcuteSV.BND."); vcf_num(S, svid); vcf_ch(S, '\t');
        vcf_ch(S, vcf_iupac(b0)); vcf_ch(S, '\t');
        if (code < 2) vcf_ch(S, b0);
        vcf_ch(S, br); vcf_put(S, V.chrom + V.chrom_off[c2], V.chrom_off[c2 + 1] - V.chrom_off[c2]); vcf_ch(S, ':'); vcf_num(S, mate); vcf_ch(S, br);
        if (code >= 2) vcf_ch(S, b0);
        qual_filter_precise();
        vcf_lit(S, ";SVTYPE=BND;RE="); vcf_num(S, re);
        rnames();
        af();                                                                           // DR '.' -> AF=. (:412-414)
    }
    tail();
    if (row) { row->chrom = ch; vcf_interval(vpos, ref_len, has_end, end_value, &row->beg, &row->end); }
}

VCF_FN vcf_i64 vcf_record_len(const VcfView& V, vcf_i64 c, int id, vcf_i64 svid)
{
    VcfSink S{nullptr, 0, 0, 1};
    vcf_record(V, c, id, svid, S, nullptr);
    return S.o;
}
VCF_FN vcf_i64 vcf_record_write(const VcfView& V, vcf_i64 c, int id, vcf_i64 svid, uint8_t* out, vcf_i64 o, int lane, int width, VcfRow* row)
{
    VcfSink S{out, o, lane, width};
    vcf_record(V, c, id, svid, S, row);
    return S.o;
}

}  // namespace csv

// ---------------------------------------------------------------------------------------- host code: csv_vcf_in -> the view
#include <vector>

namespace csv {

// The view of a csv_vcf_in with its tables in ONE block of host memory (`pack`; the device entry uploads it as it is and moves the
// view's pointers over with vcf_view_moved), the caller's three blobs left where they are, and the emission order: chromosomes by
// chrom_rank, a stable sort by bp1 within a chromosome (generate_output :252), exactly vcf_emit_impl's.
struct VcfHost {
    std::vector<char> pack;
    std::vector<vcf_i64> order;
    VcfView view;
    vcf_i64 ref_bytes = 0, alt_bytes = 0, rn_bytes = 0;
};
// CSV_OK, or CSV_E_INVALID wherever the host emitter says it - a segment or chromosome out of range, a gl_idx without a table row
// (of a filtered call too), a non-BND range outside its contig, a call whose REF bytes are not as many as its range - and for what
// the host emitter would read outside its tables: a negative INV strand code, a BND mate chromosome outside the table, a genotyped
// call whose DV and DR give no allele frequency in [0, 1].
int vcf_host_prepare(const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, VcfHost& H);
// H.view with every table pointer moved from H.pack to `base` (a copy of the block elsewhere) and the blobs at ref / alt / rn
VcfView vcf_view_moved(const VcfHost& H, const char* base, const uint8_t* ref, const uint8_t* alt, const uint8_t* rn);

}  // namespace csv
