// sam_core_main.cpp — cutesv_amd/csrc/sam_core.h on its own, for tests/test_sam_input.py: built with -fsanitize=address,undefined and
// run as it is, nothing preloaded.  Every text the core reads is a heap block of exactly its size, so a byte read too far is seen.
//   sam_core_main stream IN OUT      the SAM file IN -> the inflated BAM stream (header image and records) into OUT; every line is handed
//                                    to the line rule as a block of its own; a refusal prints "refused: <text>" and writes nothing
//   sam_core_main windows IN W       the window rule over IN with windows of W bytes: prints the cuts; they must tile the body in whole lines
//   sam_core_main numbers            the float rule against strtod on crafted and generated texts, the integer rule at its limits,
//                                    the base table, the integer tag types at their borders
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../cutesv_amd/csrc/sam_core.h"

using csv::sm_i64;

static bool slurp(const char* path, std::unique_ptr<uint8_t[]>* out, sm_i64* n)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    *n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out->reset(new uint8_t[(size_t)*n]);                  // (exactly the file)
    const bool ok = *n == 0 || fread(out->get(), 1, (size_t)*n, f) == (size_t)*n;
    fclose(f);
    return ok;
}

static int run_stream(const char* in, const char* outp)
{
    std::unique_ptr<uint8_t[]> t;
    sm_i64 n = 0;
    if (!slurp(in, &t, &n)) return 2;
    csv::SamHeader H;
    std::string err;
    if (!csv::sam_header_parse(t.get(), n, &H, &err)) { printf("refused: %s\n", err.c_str()); return 0; }
    std::vector<uint8_t> stream(H.image);
    csv::SamCounts cnt;
    sm_i64 line = H.lines;
    for (sm_i64 a = H.text_bytes; a < n; line++) {
        sm_i64 e = a;
        while (e < n && t[(size_t)e] != '\n') e++;
        std::unique_ptr<uint8_t[]> one(new uint8_t[(size_t)(e - a)]);           // the line alone, exactly its bytes
        memcpy(one.get(), t.get() + a, (size_t)(e - a));
        const int why = csv::sam_line_record(one.get(), 0, e - a, H.table(), &stream, &cnt);
        if (why) { printf("refused: %s\n", csv::sam_refusal(line + 1, why).c_str()); return 0; }
        a = e + 1;
    }
    // the window form over the whole body must give the same bytes
    std::vector<uint8_t> again(H.image);
    csv::SamCounts cnt2;
    sm_i64 lines2 = 0, bad = 0;
    if (csv::sam_window_records(t.get(), H.text_bytes, n, H.lines, H.table(), &again, &cnt2, &lines2, &bad) != csv::SAM_OK || again != stream || lines2 != line - H.lines) {
        fprintf(stderr, "the window form differs\n");
        return 1;
    }
    FILE* f = fopen(outp, "wb");
    if (!f) return 2;
    fwrite(stream.data(), 1, stream.size(), f);
    fclose(f);
    printf("ok %lld lines %lld patches %lld cg\n", (long long)(line - H.lines), (long long)cnt.patches, (long long)cnt.cg);
    return 0;
}

static int run_windows(const char* in, sm_i64 w)
{
    std::unique_ptr<uint8_t[]> t;
    sm_i64 n = 0;
    if (!slurp(in, &t, &n)) return 2;
    csv::SamHeader H;
    std::string err;
    if (!csv::sam_header_parse(t.get(), n, &H, &err)) return 1;
    for (sm_i64 w0 = H.text_bytes; w0 < n;) {
        const sm_i64 w1 = csv::sam_window_end(t.get(), n, w0, w);
        if (w1 <= w0 || w1 > n || (w1 < n && t[(size_t)w1 - 1] != '\n')) { fprintf(stderr, "cut %lld %lld\n", (long long)w0, (long long)w1); return 1; }
        printf("%lld %lld\n", (long long)w0, (long long)w1);
        w0 = w1;
    }
    return 0;
}

static int check_float(const std::string& s, long long* fast, long long* slow)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[s.size()]);
    memcpy(p.get(), s.data(), s.size());
    float f = 0;
    const int cls = csv::sam_float_text(p.get(), (sm_i64)s.size(), &f);
    if (cls == 2) {
        const float want = (float)strtod(s.c_str(), nullptr);
        if (csv::sam_float_bits(f) != csv::sam_float_bits(want)) { fprintf(stderr, "float %s: %08x, strtod %08x\n", s.c_str(), csv::sam_float_bits(f), csv::sam_float_bits(want)); return 1; }
        ++*fast;
    } else ++*slow;
    return cls;
}

static int run_numbers()
{
    long long fast = 0, slow = 0;
    const char* fast_texts[] = {"0", "-0.0", "1", "0.1", "3.14159", "123456789012345", "1e22", "1e-22", "9.5e-8", "0.000001", "16777217", "0.0123", "1E5", "+2.5e+3", "000000000000000000001.5",
                                "1.00000000000000", "8.5e0007", "123456789012345e7"};
    const char* slow_texts[] = {"1234567890123456", "1e23", "1e-40", "1e-23", "0.1234567890123456", "1e00007", "1234567890123456e1"};
    const char* no_texts[] = {"inf", "nan", "-inf", "1.", ".5", "1e", "1e+", "--1", "", "0x10", "1.5.5", "1e5e5", " 1", "1 ", "+", "e5"};
    for (const char* s : fast_texts) if (check_float(s, &fast, &slow) != 2) { fprintf(stderr, "not fast: %s\n", s); return 1; }
    for (const char* s : slow_texts) if (check_float(s, &fast, &slow) != 1) { fprintf(stderr, "not slow: %s\n", s); return 1; }
    for (const char* s : no_texts) if (check_float(s, &fast, &slow) != 0) { fprintf(stderr, "grammar: %s\n", s); return 1; }
    // generated: every digit count 1 .. 17, every exponent -25 .. 25, with and without a fraction
    unsigned long long x = 88172645463325252ull;
    for (int rep = 0; rep < 40; rep++)
        for (int nd = 1; nd <= 17; nd++)
            for (int ex = -25; ex <= 25; ex++) {
                std::string s;
                for (int k = 0; k < nd; k++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; s += (char)('0' + x % 10); }
                if (rep & 1) s.insert(s.begin(), '-');
                if (nd > 1 && (rep & 2)) s.insert(s.begin() + 1 + (rep & 1) + (int)(x % (unsigned)(nd - 1)), '.');
                if (ex) s += "e" + std::to_string(ex);
                if (check_float(s, &fast, &slow) == 0) { fprintf(stderr, "grammar: %s\n", s.c_str()); return 1; }
            }
    // integers
    sm_i64 v = 0;
    auto it = [&](const char* s, bool sign) { std::unique_ptr<uint8_t[]> p(new uint8_t[strlen(s)]); memcpy(p.get(), s, strlen(s)); return csv::sam_int_text(p.get(), (sm_i64)strlen(s), sign, &v); };
    if (!it("0", false) || v != 0 || !it("999999999999999999", false) || v != 999999999999999999ll || it("1000000000000000000", false) || it("", false) || it("-", true) || it("-5", false) ||
        !it("-5", true) || v != -5 || !it("+7", true) || v != 7 || it("1x", false) || it("1 ", false)) { fprintf(stderr, "integers\n"); return 1; }
    const long long borders[] = {-2147483649ll, -2147483648ll, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 4294967295ll, 4294967296ll};
    const char want[] = {0, 'i', 'i', 's', 's', 'c', 'c', 'C', 'C', 'S', 'S', 'I', 'I', 0};
    for (int k = 0; k < 14; k++) { int w; if (csv::sam_int_type(borders[k], &w) != want[k]) { fprintf(stderr, "type of %lld\n", borders[k]); return 1; } }
    const char table[] = "=ACMGRSVTWYHKDBN";
    for (int c = 0; c < 256; c++) {
        int want_code = 15;
        for (int k = 0; k < 16; k++) if (c == table[k] || (c >= 'a' && c <= 'z' && c - 32 == table[k])) want_code = k;
        if ((int)csv::sam_base_code((uint32_t)c) != want_code) { fprintf(stderr, "base %d\n", c); return 1; }
    }
    printf("numbers ok %lld fast %lld slow\n", fast, slow);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "stream")) return run_stream(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "windows")) return run_windows(argv[2], atoll(argv[3]));
    if (argc == 2 && !strcmp(argv[1], "numbers")) return run_numbers();
    fprintf(stderr, "usage: sam_core_main stream IN OUT | windows IN W | numbers\n");
    return 2;
}
