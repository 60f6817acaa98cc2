// vcf_core_main.cpp — csv_vcf_emit_core_host (the record core of csrc/vcf_core.h with one lane) as a stand-alone program, for the sanitizers:
//   vcf_core_main TABLE OUT
// TABLE: a csv_vcf_in with its per-call REF blob as tests/vcf_core_helpers.py's dump() writes it.  The program asks for the need with no
// capacity, then writes the records into a heap block of EXACTLY that many bytes (one byte past it is the sanitizer's to catch), checks
// that one byte less is refused with the same need and nothing written, and stores the text in OUT.  Prints "ok <bytes> <svid x 5>".
// Built by tests/test_vcf_core.py together with csrc/vcf_emit.cpp; nothing of it is loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/cutesv_hip.h"

namespace {

struct Reader {
    FILE* f;
    template <class T> std::vector<T> arr(size_t n)
    {
        std::vector<T> v(n);
        if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short table\n"); exit(2); }
        return v;
    }
    std::string str()
    {
        const int32_t n = arr<int32_t>(1)[0];
        const std::vector<char> b = arr<char>((size_t)n);
        return std::string(b.begin(), b.end());
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: vcf_core_main TABLE OUT\n"); return 2; }
    Reader r{fopen(argv[1], "rb")};
    if (!r.f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<int64_t> h = r.arr<int64_t>(8);
    const std::vector<int32_t> fl = r.arr<int32_t>(4);
    const size_t n = (size_t)h[0], n_seg = (size_t)h[1], n_chrom = (size_t)h[2], n_gl = (size_t)h[3], n_strand = (size_t)h[4];
    std::vector<int32_t> call_seg = r.arr<int32_t>(n), aux = r.arr<int32_t>(n), support = r.arr<int32_t>(n), cipos = r.arr<int32_t>(n), cilen = r.arr<int32_t>(n),
                         dr = r.arr<int32_t>(n), gl = r.arr<int32_t>(n);
    std::vector<int64_t> bp1 = r.arr<int64_t>(n), bp2 = r.arr<int64_t>(n);
    const std::vector<int32_t> svtype = r.arr<int32_t>(n_seg), chrom = r.arr<int32_t>(n_seg), genotype = r.arr<int32_t>(n_seg);
    const std::vector<int64_t> clen = r.arr<int64_t>(n_chrom);
    const std::vector<int32_t> rank = r.arr<int32_t>(n_chrom);
    std::vector<std::string> names, strands, gl_strs;
    for (size_t i = 0; i < n_chrom; i++) names.push_back(r.str());
    for (size_t i = 0; i < n_strand; i++) strands.push_back(r.str());
    for (size_t i = 0; i < n_gl; i++) gl_strs.push_back(r.str());
    const std::vector<int32_t> keys = r.arr<int32_t>(n_gl);
    std::vector<int64_t> off[3];
    std::vector<char> blob[3];
    for (int k = 0; k < 3; k++) {
        off[k] = r.arr<int64_t>(n + 1);
        blob[k] = r.arr<char>((size_t)r.arr<int64_t>(1)[0]);
    }
    std::vector<int64_t> svid = r.arr<int64_t>(5);
    fclose(r.f);

    std::vector<csv_segment> segs(n_seg);
    for (size_t k = 0; k < n_seg; k++) { memset(&segs[k], 0, sizeof(csv_segment)); segs[k].svtype = svtype[k]; segs[k].chrom = chrom[k]; segs[k].genotype = genotype[k]; }
    csv_batch_out res;
    memset(&res, 0, sizeof res);
    res.n_calls = (int64_t)n; res.cap_calls = (int64_t)n;
    res.call_seg = call_seg.data(); res.call_aux = aux.data(); res.support = support.data(); res.cipos = cipos.data(); res.cilen = cilen.data(); res.dr = dr.data();
    res.dv = support.data(); res.gl_idx = gl.data(); res.bp1 = bp1.data(); res.bp2 = bp2.data();
    res.flags = CSV_OUT_NO_SUPPORT_LIST;
    std::vector<const char*> name_p, strand_p, gl_p;
    for (const std::string& s : names) name_p.push_back(s.c_str());
    for (const std::string& s : strands) strand_p.push_back(s.c_str());
    for (const std::string& s : gl_strs) gl_p.push_back(s.c_str());
    csv_vcf_in in;
    memset(&in, 0, sizeof in);
    in.res = &res; in.seg = segs.data(); in.n_seg = (int32_t)n_seg; in.n_chrom = (int32_t)n_chrom;
    in.chrom_name = name_p.data(); in.chrom_len = clen.data(); in.chrom_rank = rank.data();
    in.ins_alt = blob[0].empty() ? "" : blob[0].data(); in.ins_alt_off = off[0].data();
    in.rnames = blob[1].empty() ? "" : blob[1].data(); in.rnames_off = off[1].data();
    in.strand_name = strand_p.data(); in.gl_key = keys.data(); in.gl_str = gl_p.data(); in.n_gl = (int32_t)n_gl;
    in.min_size = h[5]; in.max_size = h[6]; in.genotype = fl[0]; in.report_readid = fl[1]; in.ignore_sequence = fl[2];
    const char* ref = blob[2].empty() ? nullptr : blob[2].data();

    int64_t need = -1, sv[5];
    memcpy(sv, svid.data(), sizeof sv);
    int rc = csv_vcf_emit_core_host(&in, ref, off[2].data(), nullptr, 0, &need, sv);
    if (rc != CSV_E_CAPACITY || need < 0 || memcmp(sv, svid.data(), sizeof sv) != 0) { fprintf(stderr, "sizing call: rc %d need %lld\n", rc, (long long)need); return 1; }
    char* out = (char*)malloc((size_t)(need > 0 ? need : 1));
    if (need > 1) {                                                 // one byte short: the same need, nothing stored, the counters as they were
        memset(out, 0x5a, (size_t)need);
        int64_t again = -1;
        rc = csv_vcf_emit_core_host(&in, ref, off[2].data(), out, need - 1, &again, sv);
        for (int64_t i = 0; i < need; i++) if ((unsigned char)out[i] != 0x5a) { fprintf(stderr, "a refused call wrote byte %lld\n", (long long)i); return 1; }
        if (rc != CSV_E_CAPACITY || again != need || memcmp(sv, svid.data(), sizeof sv) != 0) { fprintf(stderr, "short call: rc %d need %lld\n", rc, (long long)again); return 1; }
    }
    int64_t got = -1;
    rc = csv_vcf_emit_core_host(&in, ref, off[2].data(), out, need, &got, sv);
    if (rc != CSV_OK || got != need) { fprintf(stderr, "exact call: rc %d need %lld\n", rc, (long long)got); return 1; }
    FILE* o = fopen(argv[2], "wb");
    if (!o || (need > 0 && fwrite(out, 1, (size_t)need, o) != (size_t)need) || fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    free(out);
    printf("ok %lld %lld %lld %lld %lld %lld\n", (long long)need, (long long)sv[0], (long long)sv[1], (long long)sv[2], (long long)sv[3], (long long)sv[4]);
    return 0;
}
