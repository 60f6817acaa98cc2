// sam_host.cpp — the host form of SAM text -> BAM: sam_core.h's serial line rule over line ranges on host threads,
// csv_bgzf_deflate_host over block ranges, the same file byte for byte as the device route (stage_sam.hip.h).  csv_sam_records is the
// rule over a buffer, without files.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cutesv_hip.h"
#include "sam_core.h"

using csv::sm_i64;

namespace {

thread_local csv::SamStats g_last;                       // of this thread's last csv_sam_to_bam_host

int fail(char* err, int err_cap, int rc, const std::string& text)
{
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", text.c_str());
    return rc;
}

// blocks of SAM_BLOCK bytes of s[0, len) -> BGZF blocks appended to `image`, on `threads` host threads
bool deflate_blocks(const uint8_t* s, sm_i64 len, int threads, std::vector<uint8_t>* image, sm_i64* n_blocks)
{
    const sm_i64 nb = (len + csv::SAM_BLOCK - 1) / csv::SAM_BLOCK;
    *n_blocks = nb;
    if (nb == 0) return true;
    const int T = (int)std::max<sm_i64>(1, std::min<sm_i64>(threads, nb));
    std::vector<std::vector<uint8_t>> part((size_t)T);
    std::vector<int> rc((size_t)T, 0);
    auto work = [&](int w) {
        const sm_i64 b0 = nb * w / T, b1 = nb * (w + 1) / T, k = b1 - b0;
        if (k <= 0) return;
        std::vector<int64_t> off((size_t)k);
        std::vector<int32_t> ln((size_t)k), sizes((size_t)k);
        for (sm_i64 i = 0; i < k; i++) { off[(size_t)i] = (b0 + i) * csv::SAM_BLOCK; ln[(size_t)i] = (int32_t)std::min<sm_i64>(csv::SAM_BLOCK, len - off[(size_t)i]); }
        std::vector<uint8_t>& o = part[(size_t)w];
        o.resize((size_t)(k * (csv::SAM_BLOCK + 31)));
        int64_t got = 0;
        rc[(size_t)w] = csv_bgzf_deflate_host(s, len, (int32_t)k, off.data(), ln.data(), o.data(), (int64_t)o.size(), sizes.data(), &got, nullptr);
        if (got < 0 || got > (int64_t)o.size()) rc[(size_t)w] = CSV_E_INVALID;
        o.resize(rc[(size_t)w] ? 0 : (size_t)got);
    };
    std::vector<std::thread> th;
    for (int w = 1; w < T; w++) th.emplace_back(work, w);
    work(0);
    for (auto& x : th) x.join();
    for (int w = 0; w < T; w++) {
        if (rc[(size_t)w]) return false;
        image->insert(image->end(), part[(size_t)w].begin(), part[(size_t)w].end());
    }
    return true;
}

}  // namespace

extern "C" {

int csv_sam_records(const uint8_t* text, int64_t n, int32_t n_ref, const uint8_t* name_blob, const int32_t* name_off, int64_t first_line, uint8_t* out, int64_t cap, int64_t* need,
                    int64_t* counts, char* err, int err_cap)
{
    if (n < 0 || n_ref < 0 || !need || cap < 0 || (n > 0 && !text) || (n_ref > 0 && (!name_blob || !name_off)) || (cap > 0 && !out) || first_line < 1)
        return fail(err, err_cap, CSV_E_INVALID, "bad csv_sam_records");
    *need = 0;
    // the name table: sorted here (the caller gives the header's order)
    csv::SamHeader H;
    for (int32_t i = 0; i < n_ref; i++) {
        if (name_off[i] < 0 || name_off[i + 1] < name_off[i]) return fail(err, err_cap, CSV_E_INVALID, "bad csv_sam_records: the name offsets");
        H.names.emplace_back((const char*)name_blob + name_off[i], (size_t)(name_off[i + 1] - name_off[i]));
    }
    std::vector<int32_t> order((size_t)n_ref);
    for (int32_t i = 0; i < n_ref; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return csv::sam_name_cmp((const uint8_t*)H.names[(size_t)a].data(), (sm_i64)H.names[(size_t)a].size(), (const uint8_t*)H.names[(size_t)b].data(), (sm_i64)H.names[(size_t)b].size()) < 0; });
    H.off.push_back(0);
    for (int32_t k = 0; k < n_ref; k++) {
        const std::string& s = H.names[(size_t)order[(size_t)k]];
        H.blob.insert(H.blob.end(), s.begin(), s.end()); H.off.push_back((int32_t)H.blob.size()); H.id.push_back(order[(size_t)k]);
    }
    std::vector<uint8_t> rec;
    csv::SamCounts cnt;
    sm_i64 lines = 0, bad = 0;
    const int why = csv::sam_window_records(text, 0, n, first_line - 1, H.table(), &rec, &cnt, &lines, &bad);
    if (why) return fail(err, err_cap, CSV_E_INVALID, csv::sam_refusal(bad, why));
    *need = (int64_t)rec.size();
    if (counts) { counts[0] = lines; counts[1] = cnt.patches; counts[2] = cnt.cg; }
    if ((int64_t)rec.size() > cap) return fail(err, err_cap, CSV_E_CAPACITY, "csv_sam_records: out is too small");
    if (!rec.empty()) memcpy(out, rec.data(), rec.size());
    return CSV_OK;
}

int csv_sam_to_bam_host(const char* sam_path, const char* out_path, int64_t window_bytes, int32_t threads, char* err, int err_cap)
{
    g_last = csv::SamStats();
    if (!sam_path || !out_path || window_bytes < 0 || window_bytes > csv::SAM_WINDOW_MAX || threads < 0) return fail(err, err_cap, CSV_E_INVALID, "bad csv_sam_to_bam_host");
    if (window_bytes == 0) window_bytes = csv::SAM_WINDOW;
    if (threads == 0) threads = 1;
    csv::SamStats st;
    csv::SamMap M;
    std::string text;
    if (!M.open(sam_path, &text)) return fail(err, err_cap, CSV_E_INVALID, text);
    csv::SamHeader H;
    if (!csv::sam_header_parse(M.t, M.n, &H, &text)) return fail(err, err_cap, CSV_E_INVALID, text);
    const csv::SamNames N = H.table();
    st.header_bytes = (sm_i64)H.image.size(); st.text_bytes = M.n; st.lines = H.lines;
    std::vector<uint8_t> pending(H.image), image;
    FILE* f = nullptr;
    auto finish = [&](int rc, const std::string& why) -> int {
        if (f) fclose(f);
        if (rc && f) remove(out_path);
        if (rc) return fail(err, err_cap, rc, why);
        g_last = st;
        return CSV_OK;
    };
    auto flush = [&](bool all) -> bool {                  // whole blocks (all: every byte) of `pending` -> the file
        const sm_i64 len = all ? (sm_i64)pending.size() : (sm_i64)pending.size() / csv::SAM_BLOCK * csv::SAM_BLOCK;
        if (len == 0) return true;
        image.clear();
        sm_i64 nb = 0;
        if (!deflate_blocks(pending.data(), len, threads, &image, &nb)) { text = "the stream does not deflate"; return false; }
        if (!f && !(f = fopen(out_path, "wb"))) { text = std::string("cannot write ") + out_path; return false; }
        if (fwrite(image.data(), 1, image.size(), f) != image.size()) { text = std::string("cannot write ") + out_path; return false; }
        st.blocks += nb; st.out_bytes += (sm_i64)image.size(); st.stream_bytes += len;
        pending.erase(pending.begin(), pending.begin() + len);
        return true;
    };
    for (sm_i64 w0 = H.text_bytes; w0 < M.n;) {
        const sm_i64 w1 = csv::sam_window_end(M.t, M.n, w0, window_bytes);
        if (w1 - w0 > csv::SAM_WINDOW_MAX) return finish(CSV_E_INVALID, csv::sam_refusal(st.lines + 1, csv::SAM_E_SIZE));
        // the line starts of the window, cut into one range per thread
        std::vector<sm_i64> starts;
        for (sm_i64 a = w0; a < w1;) {
            starts.push_back(a);
            const uint8_t* nl = (const uint8_t*)memchr(M.t + a, '\n', (size_t)(w1 - a));
            a = nl ? (nl - M.t) + 1 : w1;
        }
        const sm_i64 nl = (sm_i64)starts.size();
        const int T = (int)std::max<sm_i64>(1, std::min<sm_i64>(threads, nl));
        std::vector<std::vector<uint8_t>> part((size_t)T);
        std::vector<csv::SamCounts> cnt((size_t)T);
        std::vector<int> why((size_t)T, 0);
        std::vector<sm_i64> bad((size_t)T, 0);
        auto work = [&](int w) {
            const sm_i64 l0 = nl * w / T, l1 = nl * (w + 1) / T;
            if (l1 <= l0) return;
            why[(size_t)w] = csv::sam_window_records(M.t, starts[(size_t)l0], l1 < nl ? starts[(size_t)l1] : w1, st.lines + l0, N, &part[(size_t)w], &cnt[(size_t)w], nullptr, &bad[(size_t)w]);
        };
        std::vector<std::thread> th;
        for (int w = 1; w < T; w++) th.emplace_back(work, w);
        work(0);
        for (auto& x : th) x.join();
        for (int w = 0; w < T; w++)                        // (the ranges are in line order: the first refusal is the lowest line)
            if (why[(size_t)w]) return finish(CSV_E_INVALID, csv::sam_refusal(bad[(size_t)w], why[(size_t)w]));
        for (int w = 0; w < T; w++) {
            pending.insert(pending.end(), part[(size_t)w].begin(), part[(size_t)w].end());
            st.patches += cnt[(size_t)w].patches; st.cg += cnt[(size_t)w].cg;
        }
        st.lines += nl; st.records += nl; st.windows++;
        if (!flush(false)) return finish(CSV_E_INVALID, text);
        w0 = w1;
    }
    if (!flush(true)) return finish(CSV_E_INVALID, text);
    if (fwrite(csv::SAM_EOF_BLOCK, 1, sizeof csv::SAM_EOF_BLOCK, f) != sizeof csv::SAM_EOF_BLOCK) return finish(CSV_E_INVALID, std::string("cannot write ") + out_path);
    st.blocks++; st.out_bytes += (sm_i64)sizeof csv::SAM_EOF_BLOCK;
    return finish(CSV_OK, "");
}

// the stats of this thread's last csv_sam_to_bam_host (csv_sam_stats with a null context)
__attribute__((visibility("hidden"))) void csv_sam_host_last(int64_t* counts, double* ms) { csv::sam_stats_out(g_last, counts, ms); }

}  // extern "C"
