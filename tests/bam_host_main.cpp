// bam_host_main.cpp — the host route of the BAM reader (cutesv_amd/csrc/bam_host.cpp) as a stand-alone program, for the address and
// undefined-behaviour sanitizers: tests/test_bam_reader.py builds it together with bam_host.cpp with -fsanitize=address,undefined
// and the runtimes linked in (nothing is preloaded), runs it over small files and compares every line it prints with what BamFile of
// the product library reports for the same read.  The window arithmetic, the memmove of the kept tail and the memcpys into the two
// images all run here.  The device entries bam_host.cpp links against are stubs that fail: the host route never calls them.
//
//     bam_host_main FILE THREADS OP...
//       load[=PATH]            csv_bam_index_load                     -> "load ok" | "load none" | "load error: <text>"
//       drop                   csv_bam_index_drop
//       build                  csv_bam_index_build + _bytes           -> "build bytes=<n> crc=<crc32> records=<n>" | "error: <text>"
//       chunks:REFID:K         the whole contig, K records a chunk    -> one "chunk ..." line per chunk | "error: <text>"
//       region:REFID:BEG:END   one region in one chunk
//       ranges:REFID:K:B,E,... sorted, disjoint ranges, K records a chunk
//       count:REFID            count only                             -> "count <n>"
// A chunk line holds n_records, more, the sizes and the CRC32 of slim, rec_off, rec_len, host and host_off.  A file that does not
// open prints "open: <text>".  The exit status is 0 unless the command line is malformed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../include/cutesv_hip.h"
#include "../cutesv_amd/csrc/frame_core.h"
#include "../cutesv_amd/csrc/index_core.h"

// ---- the 18 library entries bam_host.cpp needs and the host route never reaches
extern "C" {
int csv_bgzf_inflate(csv_ctx*, const uint8_t*, int64_t, int32_t, const int64_t*, const int32_t*, const int64_t*, const int32_t*, const uint32_t*, uint8_t*, int64_t, int32_t, uint8_t*,
                     double*) { return CSV_E_STATE; }
int csv_host_alloc(int64_t, void**) { return CSV_E_STATE; }
void csv_host_free(void*) {}
const char* csv_last_error(const csv_ctx*) { return "a stub of bam_host_main was called"; }
}
int csv_frame_window(csv_ctx*, const uint8_t*, int64_t, int32_t, const int64_t*, const int32_t*, const int64_t*, const int32_t*, const uint32_t*, int64_t, int64_t, int64_t, uint8_t*,
                     double*) { return CSV_E_STATE; }
uint64_t csv_frame_window_serial(const csv_ctx*) { return 0; }
int csv_frame_window_put(csv_ctx*, int64_t, const uint8_t*, int64_t) { return CSV_E_STATE; }
int csv_frame_run(csv_ctx*, int32_t, const int64_t*, const int32_t*, int32_t, int64_t, const csv::FrRow**, csv::FrStitch*) { return CSV_E_STATE; }
int csv_frame_chunk_begin(csv_ctx*, const void*) { return CSV_E_STATE; }
int csv_frame_pack(csv_ctx*, int64_t, const csv::FrPack*, int64_t, int64_t) { return CSV_E_STATE; }
int csv_frame_chunk_end(csv_ctx*, int64_t, const int64_t*, const uint32_t*, const int64_t*, const int32_t*, const int32_t*) { return CSV_E_STATE; }
int csv_frame_reader(csv_ctx*, const void*, int) { return CSV_E_STATE; }
int csv_frame_fetch(csv_ctx*, const void*, uint8_t*, uint8_t*) { return CSV_E_STATE; }
int csv_frame_counters(csv_ctx*, int64_t*, int64_t*, double*, int64_t*, int64_t*, int) { return CSV_E_STATE; }
int csv_index_begin(csv_ctx*, int32_t, const csv::ix_i64*, int64_t, const csv::ix_i64*, const csv::ix_i64*, const uint32_t*) { return CSV_E_STATE; }
int csv_index_window(csv_ctx*, int64_t, int64_t, int64_t, const csv::IxCarry*, csv::IxVerdict*, const csv::IxRun**) { return CSV_E_STATE; }
int csv_index_end(csv_ctx*, csv::ix_u64*, int64_t, csv::ix_u64*, int64_t) { return CSV_E_STATE; }
int csv_index_counters(csv_ctx*, double*, int64_t*, int64_t*, int64_t*) { return CSV_E_STATE; }

static const int64_t ALL = 1ll << 62;

static unsigned crc_of(const void* p, size_t bytes) { return (unsigned)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)p, (uInt)bytes); }

// "a:b:c" -> the numbers behind the op's name; false: not `count` of them
static bool numbers(const std::string& s, char sep, size_t count, std::vector<int64_t>* out)
{
    out->clear();
    size_t at = 0;
    while (at <= s.size()) {
        size_t e = s.find(sep, at);
        if (e == std::string::npos) e = s.size();
        if (e == at) return false;
        char* stop = nullptr;
        const std::string tok = s.substr(at, e - at);
        out->push_back(strtoll(tok.c_str(), &stop, 10));
        if (*stop) return false;
        at = e + 1;
    }
    return count == 0 || out->size() == count;
}

static void print_chunk(const csv_bam_chunk& c)
{
    const size_t n = (size_t)c.n_records;
    printf("chunk n=%lld more=%d slim=%lld:%08x rec_off=%08x rec_len=%08x host=%lld:%08x host_off=%08x\n", (long long)c.n_records, (int)c.more, (long long)c.slim_bytes,
           crc_of(c.slim, (size_t)c.slim_bytes), crc_of(c.rec_off, 8 * n), crc_of(c.rec_len, 4 * n), (long long)c.host_bytes, crc_of(c.host, (size_t)c.host_bytes),
           crc_of(c.host_off, 8 * (n + 1)));
}

// one chunk sequence: the first call restarts the scan, the following ones continue while `more` says so
static void read_all(csv_bam* b, int32_t refid, const std::vector<int64_t>& beg, const std::vector<int64_t>& end, int64_t k, bool ranges, bool count_only)
{
    int32_t flags = CSV_BAM_RESTART | (count_only ? CSV_BAM_COUNT_ONLY : 0);
    long long total = 0;
    for (;;) {
        csv_bam_chunk c;
        const int rc = ranges ? csv_bam_read_ranges(b, refid, (int32_t)beg.size(), beg.data(), end.data(), k, flags, &c) : csv_bam_read(b, refid, beg[0], end[0], k, flags, &c);
        if (rc) { printf("error: %s\n", csv_bam_error(b)); return; }
        if (!count_only) print_chunk(c);
        total += c.n_records;
        if (!c.more) break;
        flags &= ~CSV_BAM_RESTART;
    }
    if (count_only) printf("count %lld\n", total);
}

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: bam_host_main FILE THREADS OP...\n"); return 2; }
    csv_bam* b = nullptr;
    char err[512] = "";
    if (csv_bam_open(argv[1], atoi(argv[2]), &b, err, (int)sizeof err) != CSV_OK) { printf("open: %s\n", err); return 0; }
    for (int a = 3; a < argc; a++) {
        const std::string op = argv[a];
        std::vector<int64_t> v;
        if (op == "load" || op.compare(0, 5, "load=") == 0) {
            const int rc = csv_bam_index_load(b, op.size() > 5 ? op.c_str() + 5 : nullptr);
            if (rc == CSV_OK) printf("load ok\n"); else if (rc == CSV_E_STATE) printf("load none\n"); else printf("load error: %s\n", csv_bam_error(b));
        } else if (op == "drop") csv_bam_index_drop(b);
        else if (op == "build") {
            int64_t n = 0, records = 0;
            if (csv_bam_index_build(b, 0, &n) != CSV_OK) { printf("error: %s\n", csv_bam_error(b)); continue; }
            std::vector<uint8_t> bytes((size_t)n);
            if (csv_bam_index_bytes(b, bytes.data(), n, &n) != CSV_OK) { printf("error: the built bytes cannot be fetched\n"); continue; }
            csv_bam_index_build_stats(b, &records, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            printf("build bytes=%lld crc=%08x records=%lld\n", (long long)n, crc_of(bytes.data(), bytes.size()), (long long)records);
        } else if (op.compare(0, 7, "chunks:") == 0 && numbers(op.substr(7), ':', 2, &v)) read_all(b, (int32_t)v[0], {-ALL}, {ALL}, v[1], false, false);
        else if (op.compare(0, 7, "region:") == 0 && numbers(op.substr(7), ':', 3, &v)) read_all(b, (int32_t)v[0], {v[1]}, {v[2]}, (1ll << 31) - 8192, false, false);
        else if (op.compare(0, 6, "count:") == 0 && numbers(op.substr(6), ':', 1, &v)) read_all(b, (int32_t)v[0], {-ALL}, {ALL}, 1ll << 30, false, true);
        else if (op.compare(0, 7, "ranges:") == 0 && op.find(':', 7) != std::string::npos && op.find(':', op.find(':', 7) + 1) != std::string::npos) {
            const size_t c2 = op.find(':', op.find(':', 7) + 1);
            std::vector<int64_t> head, beg, end;
            if (!numbers(op.substr(7, c2 - 7), ':', 2, &head) || !numbers(op.substr(c2 + 1), ',', 0, &v) || v.empty() || v.size() % 2) { fprintf(stderr, "bad op %s\n", op.c_str()); return 2; }
            for (size_t i = 0; i < v.size(); i += 2) { beg.push_back(v[i]); end.push_back(v[i + 1]); }
            read_all(b, (int32_t)head[0], beg, end, head[1], true, false);
        } else { fprintf(stderr, "bad op %s\n", op.c_str()); csv_bam_close(b); return 2; }
    }
    csv_bam_close(b);
    return 0;
}
