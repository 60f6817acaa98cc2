// bgzf_host.cpp — the host side of the BGZF writer, no GPU involved:
//   csv_bgzf_deflate_host   deflate_core.h's host form (DflOneLane) over a batch of blocks: the statement of what csv_bgzf_deflate
//                           writes, byte for byte
//   csv_tbx_build           the body of a tabix index (.tbi, before its own BGZF compression) of VCF text: one pass over the lines,
//                           assembled by index_core.h's ix::Builder - whose bytes() behind its first 8 bytes is the body of a .tbi
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/cutesv_hip.h"
#include "deflate_core.h"
#include "index_core.h"
#include "vcf_core.h"

namespace {

// The interval of a VCF data line, 0-based and half open.  The rule lives in vcf_core.h's vcf_interval (the device emitter's rows use
// it with END as a number); this is its text parser.  It restates htslib's rule for VCF from memory (nobody could run tabix against
// it): beg = POS - 1; end = the value of an END= key of INFO - at the start of INFO or behind a ';' - when that value is greater than
// beg, else beg + len(REF).
void tbx_vcf_interval(long long pos, long long ref_len, const char* info, size_t info_len, long long* beg, long long* end)
{
    csv::vcf_interval(pos, ref_len, false, 0, beg, end);
    for (size_t i = 0; i + 4 <= info_len; i++) {
        if ((i == 0 || info[i - 1] == ';') && memcmp(info + i, "END=", 4) == 0) {
            size_t j = i + 4;
            const bool neg = j < info_len && info[j] == '-';
            if (neg) j++;
            long long v = 0;
            bool digits = false;
            while (j < info_len && info[j] >= '0' && info[j] <= '9' && v < (1ll << 50)) { v = 10 * v + (info[j] - '0'); j++; digits = true; }
            if (digits && !neg) csv::vcf_interval(pos, ref_len, true, v, beg, end);
            return;                                                // (the first END= decides)
        }
    }
}

struct TbxLine { int32_t ref; long long beg, end, u0, u1; };

int tbx_fail(char* err, int32_t err_cap, long long ordinal, const char* what)            // ordinal: of the data line, from 0; -1: the call itself
{
    if (err && err_cap > 0) {
        if (ordinal < 0) snprintf(err, (size_t)err_cap, "%s", what);
        else snprintf(err, (size_t)err_cap, "cannot build the index: line %lld %s", ordinal, what);
    }
    return CSV_E_INVALID;
}

// pass 2 of both builds: the Builder, fed as the BAM index build feeds it; every record counts as mapped
int tbx_finish(const std::vector<TbxLine>& lines, const std::vector<std::string>& names, const std::vector<csv::ix_i64>& l_ref, const csv::IxBlocks& blocks, uint8_t* out, int64_t out_cap,
               int64_t* out_bytes, char* err, int32_t err_cap)
{
    csv::ix::Builder B;
    B.begin((int32_t)names.size(), l_ref.data());
    for (const TbxLine& ln : lines) {
        const csv::IxRec x = csv::ix_record(ln.beg, ln.end - ln.beg);
        // (a POS of 2^29 itself is turned away with the positions beyond it, one base before the Builder's own rule would)
        const int why = ln.beg + 1 >= csv::IX_MAX_POS ? (int)csv::IX_E_RANGE : csv::ix_refuse(ln.ref, ln.beg, x, B.n_ref, l_ref.data(), B.prev);
        if (why) return tbx_fail(err, err_cap, B.records, csv::ix_refusal_text(why));
        B.add_record(ln.ref, ln.beg, x, false, csv::ix_voff(blocks, ln.u0), csv::ix_voff(blocks, ln.u1));
    }
    std::vector<uint8_t> o;
    o.insert(o.end(), {'T', 'B', 'I', 1});
    int32_t l_nm = 0;
    for (const std::string& s : names) l_nm += (int32_t)s.size() + 1;
    for (uint32_t v : {(uint32_t)names.size(), 2u, 1u, 2u, 0u, 35u, 0u, (uint32_t)l_nm}) csv::ix::Builder::put32(o, v);
    for (const std::string& s : names) { o.insert(o.end(), s.begin(), s.end()); o.push_back(0); }
    const std::vector<uint8_t> body = B.bytes();
    o.insert(o.end(), body.begin() + 8, body.end());
    *out_bytes = (int64_t)o.size();
    if ((int64_t)o.size() <= out_cap) memcpy(out, o.data(), o.size());
    return CSV_OK;
}

}  // namespace

extern "C" {

int csv_bgzf_deflate_host(const uint8_t* in, int64_t in_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, uint8_t* out, int64_t out_cap,
                          int32_t* block_bytes, int64_t* out_bytes, int32_t* coding_bytes)
{
    if (n_blocks < 0 || in_bytes < 0 || out_cap < 0 || !out_bytes) return CSV_E_INVALID;
    if (n_blocks > 0 && (!in_off || !in_len || !block_bytes || (in_bytes > 0 && !in) || (out_cap > 0 && !out))) return CSV_E_INVALID;
    for (int32_t k = 0; k < n_blocks; k++)
        if (in_len[k] < 0 || in_len[k] > csv::DFL_MAX_IN || in_off[k] < 0 || in_off[k] > in_bytes - in_len[k]) return CSV_E_INVALID;
    *out_bytes = 0;
    if (n_blocks == 0) return CSV_OK;
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = csv::inf_crc_entry(i);
    std::vector<uint32_t> tok(csv::DFL_MAX_IN);
    std::vector<uint8_t> slots((size_t)n_blocks * csv::DFL_SLOT);
    csv::DflWork* work = (csv::DflWork*)malloc(sizeof(csv::DflWork));
    if (!work) return CSV_E_NOMEM;
    int64_t total = 0;
    for (int32_t k = 0; k < n_blocks; k++) {
        block_bytes[k] = csv::dfl_block(csv::DflOneLane(), *work, in + in_off[k], in_len[k], tok.data(), slots.data() + (size_t)k * csv::DFL_SLOT, table,
                                        coding_bytes ? coding_bytes + 3 * (size_t)k : nullptr);
        total += block_bytes[k];
    }
    free(work);
    *out_bytes = total;
    if (total > out_cap) return CSV_OK;                            // the caller learns the need, `out` stays as it is
    int64_t at = 0;
    for (int32_t k = 0; k < n_blocks; k++) { memcpy(out + at, slots.data() + (size_t)k * csv::DFL_SLOT, (size_t)block_bytes[k]); at += block_bytes[k]; }
    return CSV_OK;
}

int csv_tbx_build(const char* text, int64_t text_bytes, int64_t n_blocks, const int64_t* uoff, const int64_t* coff, const uint32_t* isize, uint8_t* out, int64_t out_cap,
                  int64_t* out_bytes, char* err, int32_t err_cap)
{
    if (err && err_cap > 0) err[0] = 0;
    if (text_bytes < 0 || n_blocks < 1 || !uoff || !coff || !isize || out_cap < 0 || !out_bytes || (text_bytes > 0 && !text) || (out_cap > 0 && !out))
        return tbx_fail(err, err_cap, -1, "bad tabix build");
    static_assert(sizeof(csv::ix_i64) == sizeof(int64_t), "the block table is handed on as it is");
    const csv::IxBlocks blocks{(const csv::ix_i64*)uoff, (const csv::ix_i64*)coff, isize, (csv::ix_i64)n_blocks};
    // pass 1: the lines, the names in order of first appearance, the farthest end per name
    std::vector<TbxLine> lines;
    std::vector<std::string> names;
    std::unordered_map<std::string, int32_t> ids;
    std::vector<csv::ix_i64> l_ref;
    for (int64_t at = 0; at < text_bytes;) {
        const char* nl = (const char*)memchr(text + at, '\n', (size_t)(text_bytes - at));
        const int64_t e = nl ? nl - text : text_bytes, next = nl ? e + 1 : text_bytes;
        if (e > at && text[at] != '#') {
            const long long ordinal = (long long)lines.size();
            const char* col[9];
            int nc = 0;
            col[nc++] = text + at;
            for (const char* p = text + at; p < text + e && nc < 9; p++) if (*p == '\t') col[nc++] = p + 1;
            if (nc < 4) return tbx_fail(err, err_cap, ordinal, "has fewer than four columns");
            const char* line_end = text + e;
            auto col_end = [&](int k) { return k + 1 < nc ? col[k + 1] - 1 : line_end; };
            long long pos = 0;
            const char* p = col[1];
            bool digits = false;
            while (p < col_end(1) && *p >= '0' && *p <= '9' && pos < (1ll << 50)) { pos = 10 * pos + (*p - '0'); p++; digits = true; }
            if (!digits || p != col_end(1)) return tbx_fail(err, err_cap, ordinal, "has no numeric POS");
            TbxLine ln;
            tbx_vcf_interval(pos, (long long)(col_end(3) - col[3]), nc > 7 ? col[7] : line_end, nc > 7 ? (size_t)(col_end(7) - col[7]) : 0, &ln.beg, &ln.end);
            const std::string name(col[0], (size_t)(col_end(0) - col[0]));
            auto it = ids.find(name);
            if (it == ids.end()) { it = ids.emplace(name, (int32_t)names.size()).first; names.push_back(name); l_ref.push_back(1); }
            ln.ref = it->second; ln.u0 = at; ln.u1 = next;
            const csv::IxRec x = csv::ix_record(ln.beg, ln.end - ln.beg);
            if (x.end > l_ref[(size_t)ln.ref]) l_ref[(size_t)ln.ref] = x.end < csv::IX_MAX_POS ? x.end : csv::IX_MAX_POS;
            lines.push_back(ln);
        }
        at = next;
    }
    return tbx_finish(lines, names, l_ref, blocks, out, out_cap, out_bytes, err, err_cap);
}

int csv_tbx_build_rows(const char* names_blob, const int64_t* name_off, int32_t n_names, const int64_t* rows, int64_t n_rows, int64_t text_bytes, int64_t n_blocks, const int64_t* uoff,
                       const int64_t* coff, const uint32_t* isize, uint8_t* out, int64_t out_cap, int64_t* out_bytes, char* err, int32_t err_cap)
{
    if (err && err_cap > 0) err[0] = 0;
    if (text_bytes < 0 || n_blocks < 1 || !uoff || !coff || !isize || out_cap < 0 || !out_bytes || (out_cap > 0 && !out) || n_names < 0 || n_rows < 0 || (n_names > 0 && !name_off) ||
        (n_rows > 0 && !rows))
        return tbx_fail(err, err_cap, -1, "bad tabix build");
    const csv::IxBlocks blocks{(const csv::ix_i64*)uoff, (const csv::ix_i64*)coff, isize, (csv::ix_i64)n_blocks};
    std::vector<std::string> names;
    for (int32_t k = 0; k < n_names; k++) {
        if (name_off[k] < 0 || name_off[k + 1] < name_off[k] || (name_off[k + 1] > name_off[k] && !names_blob)) return tbx_fail(err, err_cap, -1, "bad tabix build");
        names.emplace_back(names_blob + name_off[k], (size_t)(name_off[k + 1] - name_off[k]));
    }
    // pass 1 from the rows: the lines, the farthest end per name
    std::vector<TbxLine> lines((size_t)n_rows);
    std::vector<csv::ix_i64> l_ref((size_t)n_names, 1);
    for (int64_t r = 0; r < n_rows; r++) {
        const int64_t* w = rows + 4 * r;
        const int64_t u1 = r + 1 < n_rows ? w[7] : text_bytes;
        if (w[0] < 0 || w[0] >= n_names || w[3] < 0 || u1 < w[3] || u1 > text_bytes) return tbx_fail(err, err_cap, -1, "bad tabix build");
        TbxLine& ln = lines[(size_t)r];
        ln.ref = (int32_t)w[0]; ln.beg = w[1]; ln.end = w[2]; ln.u0 = w[3]; ln.u1 = u1;
        const csv::IxRec x = csv::ix_record(ln.beg, ln.end - ln.beg);
        if (x.end > l_ref[(size_t)ln.ref]) l_ref[(size_t)ln.ref] = x.end < csv::IX_MAX_POS ? x.end : csv::IX_MAX_POS;
    }
    return tbx_finish(lines, names, l_ref, blocks, out, out_cap, out_bytes, err, err_cap);
    return CSV_OK;
}

}  // extern "C"
