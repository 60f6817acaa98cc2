// vcf_emit.cpp — host side of the stage's OUTPUT boundary: calls (structure of arrays) -> VCF body text.
// Restates generate_output (cuteSV_genotype.py:242-467) and the SVID numbering of main_ctrl
// (cuteSV main script :1208-1237) on the csv_batch_out layout; see include/cutesv_hip.h.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <unistd.h>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cutesv_hip.h"
#include "soa_access.h"
#include "ref_core.h"
#include "vcf_core.h"

namespace {

// text of the records a worker thread formats: a growable buffer that belongs to the THREAD and keeps its capacity from call to
// call (a fresh std::string per slice meant ~30 MB of new pages per emission once the records carry their REF sequences: page
// faults under the process's memory-map lock, on 16 threads at once, were most of the emitter's time)
struct Sink {
    std::string& buf;
    void put(const char* s, size_t len) { buf.append(s, len); }
    void put(const char* s) { buf.append(s); }
    void put(const std::string& s) { buf.append(s); }
    void put(char c) { buf.push_back(c); }
    void num(long long v)                                  // decimal text (snprintf was a third of the emitter's time)
    {
        char b[24];
        int k = 24;
        unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do { b[--k] = (char)('0' + u % 10); u /= 10; } while (u);
        if (v < 0) b[--k] = '-';
        buf.append(b + k, (size_t)(24 - k));
    }
};

// trans_table = str.maketrans('RYSWKMBDHV', 'ACCAGACAAA')   (cuteSV_genotype.py:262)
inline char iupac(char c)
{
    switch (c) {
    case 'R': return 'A'; case 'Y': return 'C'; case 'S': return 'C'; case 'W': return 'A'; case 'K': return 'G';
    case 'M': return 'A'; case 'B': return 'C'; case 'D': return 'A'; case 'H': return 'A'; case 'V': return 'A';
    default: return c;
    }
}

struct IupacTable { char t[256]; IupacTable() { for (int c = 0; c < 256; c++) t[c] = iupac((char)c); } };
const IupacTable kIupac;

// str(round(dv / (dv + dr), 4))  (cuteSV_genotype.py:284): correctly rounded to 4 decimals, then Python's
// shortest repr, which for such a value is the 4-decimal string without trailing zeros (one decimal kept).
void put_af(Sink& o, long long dv, long long dr)
{
    char b[32];
    int k = snprintf(b, sizeof b, "%.4f", (double)dv / (double)(dv + dr));
    while (k > 0 && b[k - 1] == '0' && b[k - 2] != '.') k--;
    o.put(b, (size_t)k);
}

struct GlRow { const char* gt; size_t gt_n; const char* pl; size_t pl_n; const char* gq; size_t gq_n; const char* qual; size_t qual_n; };

bool split_gl(const char* s, GlRow& r)
{
    const char* t1 = strchr(s, '\t'); if (!t1) return false;
    const char* t2 = strchr(t1 + 1, '\t'); if (!t2) return false;
    const char* t3 = strchr(t2 + 1, '\t'); if (!t3) return false;
    r.gt = s; r.gt_n = (size_t)(t1 - s);
    r.pl = t1 + 1; r.pl_n = (size_t)(t2 - t1 - 1);
    r.gq = t2 + 1; r.gq_n = (size_t)(t3 - t2 - 1);
    r.qual = t3 + 1; r.qual_n = strlen(t3 + 1);
    return true;
}

}  // namespace

// Records are formatted by worker threads, one slice of a chromosome's sorted calls at a time; the SVID counters a slice
// starts with are the numbers of records of each type EMITTED before it (generate_output's size filters decide that), found
// by a first pass over the slices.  Order of the text: chromosomes by name rank, records by position, as the reference writes.
namespace {
constexpr int64_t VCF_SLICE = 1024;                    // calls per work item
enum { ID_INS = csv::VCF_ID_INS, ID_DEL = csv::VCF_ID_DEL, ID_BND = csv::VCF_ID_BND, ID_DUP = csv::VCF_ID_DUP, ID_INV = csv::VCF_ID_INV };

// size filters of generate_output: the rule is vcf_core.h's (ONE definition, for this emitter and for the device's)
inline int emitted_id(const csv_vcf_in* in, const csv_batch_out& R, int64_t c)
{
    return csv::vcf_emitted_id(in->seg[R.call_seg[c]].svtype, csv_soa::bp1(R, c), csv_soa::bp2(R, c), in->min_size, in->max_size);
}

// where the reference bases of the records come from: the contigs of csv_vcf_in (blob == NULL), or - csv_vcf_emit_ref - per call
// the bases of its range, back to back: call c's are blob[off[c] .. off[c + 1])
struct RefSrc { const char* blob; const int64_t* off; };

// The contig bases the record of call c reads: [b, e), of which a DEL record prints [b, slice_e) as its REF.  ONE definition
// (vcf_core.h's vcf_ref_range), for emit_slice, for csv_vcf_ref_ranges and for the device emitter.  Empty (b == e): a call the size
// filters drop, or INS / DEL under ignore_sequence.  slen: the contig's length, 0 for a contig without sequence; a range that is not
// inside [0, slen) is the caller's to judge ('N' for BND, CSV_E_INVALID otherwise).
typedef csv::VcfRefRange RefRange;
inline RefRange call_ref_range(const csv_vcf_in* in, const csv_batch_out& R, int64_t c, int64_t slen)
{
    const int id = emitted_id(in, R, c), type = in->seg[R.call_seg[c]].svtype;
    const bool pp = id >= 0 && type == CSV_INV && strcmp(in->strand_name[csv_soa::call_aux(R, c)], "++") == 0;    // :360-365
    return csv::vcf_ref_range(id, type, in->ignore_sequence != 0, csv_soa::bp1(R, c), csv_soa::bp2(R, c), csv_soa::call_aux(R, c), pp, slen);
}
inline bool ref_range_inside(const RefRange& r, int64_t slen) { return r.b >= 0 && r.e <= slen; }

int emit_slice(const csv_vcf_in* in, const RefSrc& src, const int64_t* v, int64_t nv, int ch, int64_t* svid, Sink& o);

// A team of worker threads that lives as long as the process (thread creation is ~30 us: 15 fresh threads per call were a third
// of a 1.4 ms emission).  Between calls the workers sleep on a condition variable; inside a call (wake() .. park()) they spin
// with yield() between the three parallel loops.  run(n, f): f(i) for i in [0, n) dealt dynamically; returns when all are done.
class Team {
public:
    explicit Team(int nthreads) : n_(nthreads < 1 ? 1 : nthreads)
    {
        for (int t = 1; t < n_; t++) th_.emplace_back([this] { loop(); });
    }
    ~Team()
    {
        { std::lock_guard<std::mutex> g(m_); quit_.store(true); active_.store(true); gen_.fetch_add(1); }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int size() const { return n_; }
    void wake() { { std::lock_guard<std::mutex> g(m_); active_.store(true); } cv_.notify_all(); }
    void park() { active_.store(false); }
    template <class F> void run(int64_t n, F&& f)
    {
        if (n <= 0) return;
        std::function<void(int64_t)> fn = f;
        fn_ = &fn; total_ = n; next_.store(0); done_.store(0);
        gen_.fetch_add(1);                                  // release the workers
        work();
        while (done_.load() < n_) std::this_thread::yield();
    }
private:
    void work() { for (int64_t i; (i = next_.fetch_add(1)) < total_;) (*fn_)(i); done_.fetch_add(1); }
    void loop()
    {
        for (int seen = 0;;) {
            int g;
            while ((g = gen_.load()) == seen) {
                if (!active_.load()) {
                    std::unique_lock<std::mutex> lk(m_);
                    cv_.wait(lk, [&] { return active_.load() || quit_.load(); });
                } else std::this_thread::yield();
            }
            seen = g;
            if (quit_.load()) return;
            work();
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::atomic<int> gen_{0}, done_{0};
    std::atomic<bool> quit_{false}, active_{false};
    std::atomic<int64_t> next_{0};
    int64_t total_ = 0;
    std::function<void(int64_t)>* fn_ = nullptr;
};

// the process's team (a forked child starts its own: threads do not survive fork); one emission at a time uses it
std::mutex g_team_mu;
Team* g_team = nullptr;
int g_team_pid = 0, g_team_n = 0;
struct TeamLease {
    Team* t = nullptr; bool own = false; std::unique_lock<std::mutex> lk;
    explicit TeamLease(int nthreads)
    {
        if (nthreads <= 1) { t = new Team(1); own = true; return; }
        lk = std::unique_lock<std::mutex>(g_team_mu, std::try_to_lock);
        if (!lk.owns_lock()) { t = new Team(nthreads); own = true; t->wake(); return; }     // (another thread is emitting: a team of its own)
        const int pid = (int)getpid();
        if (!g_team || g_team_pid != pid || g_team_n != nthreads) {
            if (g_team && g_team_pid == pid) delete g_team;      // (after a fork the parent's object is just forgotten: its threads are not ours)
            g_team = new Team(nthreads); g_team_pid = pid; g_team_n = nthreads;
        }
        t = g_team; t->wake();
    }
    ~TeamLease() { if (own) delete t; else if (t) t->park(); }
};
}  // namespace

namespace {
int vcf_emit_impl(const csv_vcf_in* in, const RefSrc& src, char* out, int64_t cap, int64_t* n_written, int64_t* svid)
{
    if (!in || !in->res || !n_written || !svid) return CSV_E_INVALID;
    const csv_batch_out& R = *in->res;
    const int64_t nc = R.n_calls;
    int nthreads = (int)std::thread::hardware_concurrency();
    if (const char* e = getenv("CSV_VCF_THREADS")) nthreads = atoi(e);
    if (nthreads > 16) nthreads = 16;
    if (nthreads < 1 || nc < 2 * VCF_SLICE) nthreads = 1;
    TeamLease lease(nthreads);
    Team& team = *lease.t;

    // calls per chromosome in the order main_ctrl concatenates task results (the call order of the batch): counting sort
    std::vector<int64_t> coff((size_t)in->n_chrom + 1, 0), idx((size_t)nc);
    for (int64_t c = 0; c < nc; c++) {
        const int k = R.call_seg[c];
        if (k < 0 || k >= in->n_seg) return CSV_E_INVALID;
        const int ch = in->seg[k].chrom;
        if (ch < 0 || ch >= in->n_chrom) return CSV_E_INVALID;
        coff[(size_t)ch + 1]++;
    }
    for (int i = 0; i < in->n_chrom; i++) coff[(size_t)i + 1] += coff[(size_t)i];
    {
        std::vector<int64_t> fill(coff.begin(), coff.end() - 1);
        for (int64_t c = 0; c < nc; c++) idx[(size_t)fill[(size_t)in->seg[R.call_seg[c]].chrom]++] = c;
    }
    std::vector<int> order(in->n_chrom);
    for (int i = 0; i < in->n_chrom; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return in->chrom_rank[x] < in->chrom_rank[y]; });
    // generate_output's stable sort by int(row[2]) per chromosome (cuteSV_genotype.py:252)
    team.run(in->n_chrom, [&](int64_t ch) {
        std::stable_sort(idx.begin() + coff[(size_t)ch], idx.begin() + coff[(size_t)ch + 1], [&](int64_t x, int64_t y) { return csv_soa::bp1(R, x) < csv_soa::bp1(R, y); });
    });
    // slices in emission order
    struct Slice { int ch; int64_t lo, hi; int64_t cnt[5]; int64_t start[5]; int rc; const std::string* buf; size_t off, len; };
    static std::atomic<uint64_t> g_call{0};
    const uint64_t call_id = g_call.fetch_add(1) + 1;
    std::vector<Slice> sl;
    for (int ch : order)
        for (int64_t lo = coff[(size_t)ch]; lo < coff[(size_t)ch + 1]; lo += VCF_SLICE) {
            Slice x{};
            x.ch = ch; x.lo = lo; x.hi = lo + VCF_SLICE < coff[(size_t)ch + 1] ? lo + VCF_SLICE : coff[(size_t)ch + 1];
            sl.push_back(std::move(x));
        }
    // records per type every slice emits -> the counters it starts with (main script :1208-1237: one counter per type over the
    // whole file)
    team.run((int64_t)sl.size(), [&](int64_t i) {
        Slice& x = sl[(size_t)i];
        for (int64_t q = x.lo; q < x.hi; q++) { const int id = emitted_id(in, R, idx[(size_t)q]); if (id >= 0) x.cnt[id]++; }
    });
    int64_t run[5] = {svid[0], svid[1], svid[2], svid[3], svid[4]};
    for (Slice& x : sl) for (int t = 0; t < 5; t++) { x.start[t] = run[t]; run[t] += x.cnt[t]; }
    team.run((int64_t)sl.size(), [&](int64_t i) {
        Slice& x = sl[(size_t)i];
        static thread_local std::string tl_buf;
        static thread_local uint64_t tl_call = 0;
        if (tl_call != call_id) { tl_buf.clear(); tl_call = call_id; }         // (capacity kept)
        Sink o{tl_buf};
        x.buf = &tl_buf; x.off = tl_buf.size();
        int64_t sv[5] = {x.start[0], x.start[1], x.start[2], x.start[3], x.start[4]};
        x.rc = emit_slice(in, src, idx.data() + x.lo, x.hi - x.lo, x.ch, sv, o);
        x.len = tl_buf.size() - x.off;
    });
    int64_t total = 0;
    for (Slice& x : sl) { if (x.rc != CSV_OK) return x.rc; total += (int64_t)x.len; }
    *n_written = total;
    if (!out || total > cap) return CSV_E_CAPACITY;
    std::vector<int64_t> toff(sl.size() + 1, 0);
    for (size_t i = 0; i < sl.size(); i++) toff[i + 1] = toff[i] + (int64_t)sl[i].len;
    team.run((int64_t)sl.size(), [&](int64_t i) { const Slice& x = sl[(size_t)i]; memcpy(out + toff[(size_t)i], x.buf->data() + x.off, x.len); });
    for (int t = 0; t < 5; t++) svid[t] = run[t];
    return CSV_OK;
}
}  // namespace

extern "C" int csv_vcf_emit(const csv_vcf_in* in, char* out, int64_t cap, int64_t* n_written, int64_t* svid)
{
    return vcf_emit_impl(in, RefSrc{nullptr, nullptr}, out, cap, n_written, svid);
}

// csv_vcf_emit with the reference bases of call c taken from ref_blob[ref_off[c] .. ref_off[c + 1]): the bases of the range
// csv_vcf_ref_ranges gives for it (a BND call without a readable base, and every call without a range: no bytes)
extern "C" int csv_vcf_emit_ref(const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, char* out, int64_t cap, int64_t* n_written, int64_t* svid)
{
    static const char kNone = 0;
    if (!ref_off) return CSV_E_INVALID;
    return vcf_emit_impl(in, RefSrc{ref_blob ? ref_blob : &kNone, ref_off}, out, cap, n_written, svid);
}

// per call the contig (index into chrom_name) and the bases [beg, end) of it that the call's record reads (call_ref_range)
extern "C" int csv_vcf_ref_ranges(const csv_vcf_in* in, int64_t* beg, int64_t* end, int32_t* chrom)
{
    if (!in || !in->res) return CSV_E_INVALID;
    const csv_batch_out& R = *in->res;
    if (R.n_calls > 0 && (!beg || !end || !chrom)) return CSV_E_INVALID;
    for (int64_t c = 0; c < R.n_calls; c++) {
        const int k = R.call_seg[c];
        if (k < 0 || k >= in->n_seg) return CSV_E_INVALID;
        const int ch = in->seg[k].chrom;
        if (ch < 0 || ch >= in->n_chrom) return CSV_E_INVALID;
        const int64_t slen = in->chrom_len ? in->chrom_len[ch] : 0;
        RefRange r = call_ref_range(in, R, c, slen);
        if (r.e > r.b && !ref_range_inside(r, slen)) {
            if (!r.bnd) return CSV_E_INVALID;                                            // what csv_vcf_emit answers for it
            r.b = r.e = 0;                                                              // try/except -> 'N' (:431-434)
        }
        beg[c] = r.b; end[c] = r.e; chrom[c] = ch;
    }
    return CSV_OK;
}

namespace {
// the records of the calls v[0 .. nv) of chromosome ch, in that order; svid: the counters to start with
int emit_slice(const csv_vcf_in* in, const RefSrc& src, const int64_t* v, int64_t nv, int ch, int64_t* svid, Sink& o)
{
    const csv_batch_out& R = *in->res;
    static const char* kFormat = "GT:DR:DV:PL:GQ";
    {
        const char* seq = (!src.blob && in->chrom_seq) ? in->chrom_seq[ch] : nullptr;
        const int64_t clen = in->chrom_len ? in->chrom_len[ch] : 0;
        const int64_t slen = (src.blob || seq) ? clen : 0;                              // (a contig without sequence has no base to read)
        const char* cname = in->chrom_name[ch];
        // a contig read straight from a FASTA file (mmap): line_bases bases, then the line break, per line of line_width bytes
        const int64_t lb = (in->chrom_line_bases && in->chrom_line_width) ? in->chrom_line_bases[ch] : 0;
        const int64_t lw = lb > 0 ? in->chrom_line_width[ch] : 0;
        for (int64_t qi = 0; qi < nv; qi++) {
            const int64_t c = v[qi];
            const csv_segment& sg = in->seg[R.call_seg[c]];
            const int type = sg.svtype;
            // TRA calls whose count_coverage gave up carry the '.' fields too (cuteSV_resolveTRA.py:276-281)
            const bool gt_on = sg.genotype != 0 && csv_soa::gl_idx(R, c) >= 0;
            // genotype strings of the row ('.' fields when the task was not genotyped)
            GlRow g{"./.", 3, ".,.,.", 5, ".", 1, ".", 1};
            if (gt_on) {
                const int32_t key = csv_soa::gl_idx(R, c);
                const int32_t* it = std::lower_bound(in->gl_key, in->gl_key + in->n_gl, key);
                if (it == in->gl_key + in->n_gl || *it != key || !split_gl(in->gl_str[it - in->gl_key], g)) return CSV_E_INVALID;
            }
            const bool imprecise = g.gt_n == 3 && memcmp(g.gt, "0/0", 3) == 0;
            // filter label (cuteSV_genotype.py:289-292)
            const char* filt = "PASS";
            if (!(g.qual_n == 1 && g.qual[0] == '.')) filt = strtod(std::string(g.qual, g.qual_n).c_str(), nullptr) >= 5.0 ? "PASS" : "q5";
            const long long pos = csv_soa::bp1(R, c), re = R.support[c];
            if (emitted_id(in, R, c) < 0) continue;                                     // the size filters (:265-268, 315-316, 351-352)
            const RefRange rr = call_ref_range(in, R, c, slen);
            const bool readable = rr.e > rr.b && ref_range_inside(rr, slen);
            if (rr.e > rr.b && !readable && !rr.bnd) return CSV_E_INVALID;               // a reference sequence is missing or too short
            const char* mine = nullptr;                                                 // csv_vcf_emit_ref: the bases of [rr.b, rr.e)
            if (src.blob) {
                if (src.off[c + 1] - src.off[c] != (readable ? rr.e - rr.b : 0)) return CSV_E_INVALID;
                mine = src.blob + src.off[c];
            }
            auto at = [&](int64_t i) -> char { return mine ? mine[i - rr.b] : lb > 0 ? seq[(i / lb) * lw + i % lb] : seq[i]; };
            auto put_rnames = [&]() {
                if (in->report_readid) { o.put(";RNAMES="); if (in->rnames) o.put(in->rnames + in->rnames_off[c], (size_t)(in->rnames_off[c + 1] - in->rnames_off[c])); }
            };
            auto put_af_field = [&](bool numeric) {
                if (!in->genotype) return;
                o.put(";AF=");
                if (numeric) put_af(o, re, csv_soa::dr(R, c)); else o.put('.');
            };
            auto put_tail = [&]() {           // QUAL FILTER INFO are written by the caller; this is FORMAT + sample
                o.put('\t'); o.put(kFormat); o.put('\t');
                o.put(g.gt, g.gt_n); o.put(':');
                if (gt_on) o.num(csv_soa::dr(R, c)); else o.put('.');
                o.put(':'); o.num(re); o.put(':'); o.put(g.pl, g.pl_n); o.put(':'); o.put(g.gq, g.gq_n); o.put('\n');
            };
            if (type == CSV_DEL || type == CSV_INS) {
                const long long len = csv_soa::bp2(R, c);                                         // |SVLEN|
                const long long end = type == CSV_INS ? pos : pos + len;
                const long long r0 = rr.b;
                o.put(cname); o.put('\t'); o.num(pos); o.put('\t');
                o.put(type == CSV_INS ? "cuteSV.INS." : "cuteSV.DEL."); o.num(svid[type == CSV_INS ? ID_INS : ID_DEL]++); o.put('\t');
                if (in->ignore_sequence) {
                    o.put("N\t"); o.put(type == CSV_INS ? "<INS>" : "<DEL>");
                } else if (type == CSV_INS) {
                    const char b0 = at(r0);                                             // ref_chrom[max(pos-1, 0)] (:297)
                    o.put(iupac(b0)); o.put('\t'); o.put(b0);
                    if (in->ins_alt) o.put(in->ins_alt + in->ins_alt_off[c], (size_t)(in->ins_alt_off[c + 1] - in->ins_alt_off[c]));
                } else {
                    const long long r1 = rr.slice_e;                                    // slice end, clamped like Python
                    // the deleted bases: whole runs of a FASTA line at a time (memcpy), then the IUPAC table over the copy
                    // (a call, a division and a push_back per base made this slice 95 % of the emitter's time on a 30x genome)
                    if (r1 > r0) {
                        const size_t w0 = o.buf.size();
                        o.buf.resize(w0 + (size_t)(r1 - r0));
                        char* dst = &o.buf[w0];
                        if (mine) memcpy(dst, mine, (size_t)(r1 - r0));
                        else if (lb > 0) {
                            long long i = r0;
                            while (i < r1) {
                                const long long in_line = i % lb, run = std::min<long long>(lb - in_line, r1 - i);
                                memcpy(dst, seq + (i / lb) * lw + in_line, (size_t)run);
                                dst += run; i += run;
                            }
                        } else memcpy(dst, seq + r0, (size_t)(r1 - r0));
                        char* p = &o.buf[w0];
                        for (long long k = 0; k < r1 - r0; k++) p[k] = kIupac.t[(unsigned char)p[k]];
                    }
                    o.put('\t');
                    o.put(at(r0));
                }
                o.put('\t'); o.put(g.qual, g.qual_n); o.put('\t'); o.put(filt); o.put('\t');
                o.put(imprecise ? "IMPRECISE" : "PRECISE");
                o.put(type == CSV_INS ? ";SVTYPE=INS;SVLEN=" : ";SVTYPE=DEL;SVLEN=");
                o.num(type == CSV_INS ? len : -len);
                o.put(";END="); o.num(end);
                o.put(";CIPOS=-"); o.num(csv_soa::cipos(R, c)); o.put(','); o.num(csv_soa::cipos(R, c));
                o.put(";CILEN=-"); o.num(csv_soa::cilen(R, c)); o.put(','); o.num(csv_soa::cilen(R, c));
                o.put(";RE="); o.num(re);
                put_rnames();
                put_af_field(gt_on);
                if (type == CSV_DEL) o.put(";STRAND=+-");
                put_tail();
            } else if (type == CSV_DUP) {
                const long long len = csv_soa::bp2(R, c) - csv_soa::bp1(R, c);
                const char b0 = at(rr.b);                                               // ref_chrom[int(i[2])] (:334)
                o.put(cname); o.put('\t'); o.num(pos + 1); o.put('\t');
                o.put("cuteSV.DUP."); o.num(svid[ID_DUP]++); o.put('\t');
                o.put(iupac(b0)); o.put("\t<DUP>\t");
                o.put(g.qual, g.qual_n); o.put('\t'); o.put(filt); o.put('\t');
                o.put(imprecise ? "IMPRECISE" : "PRECISE");
                o.put(";SVTYPE=DUP;SVLEN="); o.num(len);
                o.put(";END="); o.num(pos + 1 + llabs(len));
                o.put(";RE="); o.num(re); o.put(";STRAND=-+");
                put_rnames();
                put_af_field(gt_on);
                put_tail();
            } else if (type == CSV_INV) {
                const long long len = csv_soa::bp2(R, c) - csv_soa::bp1(R, c);
                const char* strand = in->strand_name[csv_soa::call_aux(R, c)];
                const bool pp = strcmp(strand, "++") == 0;                              // :360-365
                const long long pinv = pp ? pos : pos + 1;
                const char b0 = at(rr.b);
                o.put(cname); o.put('\t'); o.num(pinv); o.put('\t');
                o.put("cuteSV.INV."); o.num(svid[ID_INV]++); o.put('\t');
                o.put(iupac(b0)); o.put("\t<INV>\t");
                o.put(g.qual, g.qual_n); o.put('\t'); o.put(filt); o.put('\t');
                o.put(imprecise ? "IMPRECISE" : "PRECISE");
                o.put(";SVTYPE=INV;SVLEN="); o.num(len);
                o.put(";END="); o.num(pinv + llabs(len));
                o.put(";RE="); o.num(re); o.put(";STRAND="); o.put(strand);
                put_rnames();
                put_af_field(gt_on);
                put_tail();
            } else {                                                                    // BND (:400-458)
                const int code = csv_soa::call_aux(R, c) & 7;
                const char* chr2 = in->chrom_name[csv_soa::call_aux(R, c) >> 3];
                const long long mate = csv_soa::bp2(R, c) + ((code == 0 || code == 2) ? 1 : 0);    // TRA:140
                const bool nfirst = code < 2;                                           // ALT starts with 'N' (types A/B)
                const long long pbnd = nfirst ? pos : pos + 1;
                const char b0 = readable ? at(rr.b) : 'N';                              // try/except -> 'N' (:431-434)
                o.put(cname); o.put('\t'); o.num(pbnd); o.put('\t');
                o.put("cuteSV.BND."); o.num(svid[ID_BND]++); o.put('\t');
                o.put(iupac(b0)); o.put('\t');
                char mt[64];
                const int mk = snprintf(mt, sizeof mt, ":%lld", mate);
                if (code == 0) { o.put(b0); o.put('['); o.put(chr2); o.put(mt, (size_t)mk); o.put('['); }
                else if (code == 1) { o.put(b0); o.put(']'); o.put(chr2); o.put(mt, (size_t)mk); o.put(']'); }
                else if (code == 2) { o.put('['); o.put(chr2); o.put(mt, (size_t)mk); o.put('['); o.put(b0); }
                else { o.put(']'); o.put(chr2); o.put(mt, (size_t)mk); o.put(']'); o.put(b0); }
                o.put('\t'); o.put(g.qual, g.qual_n); o.put('\t'); o.put(filt); o.put('\t');
                o.put(imprecise ? "IMPRECISE" : "PRECISE");
                o.put(";SVTYPE=BND;RE="); o.num(re);
                put_rnames();
                put_af_field(gt_on);                                                    // DR '.' -> AF=. (:412-414)
                put_tail();
            }
        }
    }
    return CSV_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------- the record core (vcf_core.h)
// csv_vcf_in -> the flat view the record core reads, checked: what csv_vcf_emit_core_host and csv_vcf_emit_device (stage_vcf_emit.hip.h)
// both start with.  Everything the core trusts is judged here, before a byte is written or a kernel launched.
namespace csv {

int vcf_host_prepare(const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, VcfHost& H)
{
    if (!in || !in->res || !ref_off || in->n_seg < 0 || in->n_chrom < 0 || in->n_gl < 0) return CSV_E_INVALID;
    const csv_batch_out& R = *in->res;
    const int64_t nc = R.n_calls;
    if (nc < 0 || (nc > 0 && (!R.call_seg || !R.bp1 || !R.bp2 || !R.support || !in->seg))) return CSV_E_INVALID;
    if ((in->n_chrom > 0 && (!in->chrom_name || !in->chrom_rank)) || (in->n_gl > 0 && (!in->gl_key || !in->gl_str))) return CSV_E_INVALID;
    const bool with_alt = in->ins_alt && in->ins_alt_off && !in->ignore_sequence, with_rn = in->report_readid && in->rnames && in->rnames_off;
    // the genotype table: the four strings of every key back to back, and the two facts the records need of them
    std::vector<int32_t> gl_off{0};
    std::vector<uint8_t> gl, gl_flag((size_t)in->n_gl, 0);
    std::vector<char> gl_ok((size_t)in->n_gl, 0);
    for (int r = 0; r < in->n_gl; r++) {
        GlRow g{};
        const bool ok = in->gl_str[r] && split_gl(in->gl_str[r], g);
        gl_ok[(size_t)r] = ok;
        const char* f[4] = {g.gt, g.pl, g.gq, g.qual};
        const size_t fn[4] = {g.gt_n, g.pl_n, g.gq_n, g.qual_n};
        for (int k = 0; k < 4; k++) {
            if (ok) gl.insert(gl.end(), f[k], f[k] + fn[k]);
            gl_off.push_back((int32_t)gl.size());
        }
        if (!ok) continue;
        const bool q5 = !(g.qual_n == 1 && g.qual[0] == '.') && strtod(std::string(g.qual, g.qual_n).c_str(), nullptr) < 5.0;      // (cuteSV_genotype.py:289-292)
        gl_flag[(size_t)r] = (uint8_t)((q5 ? 1 : 0) | ((g.gt_n == 3 && memcmp(g.gt, "0/0", 3) == 0) ? 2 : 0));
    }
    // the calls, every one judged; the columns as the core reads them
    std::vector<int32_t> c32((size_t)nc * 7);
    std::vector<int64_t> c64((size_t)nc * 2 + 3 * ((size_t)nc + 1), 0);
    int32_t *o_seg = c32.data(), *o_aux = o_seg + nc, *o_sup = o_aux + nc, *o_cip = o_sup + nc, *o_cil = o_cip + nc, *o_dr = o_cil + nc, *o_gl = o_dr + nc;
    int64_t *o_bp1 = c64.data(), *o_bp2 = o_bp1 + nc, *o_ref = o_bp2 + nc, *o_alt = o_ref + nc + 1, *o_rn = o_alt + nc + 1;
    int n_strand = 0;
    H.ref_bytes = H.alt_bytes = H.rn_bytes = 0;
    for (int64_t c = 0; c < nc; c++) {
        const int k = R.call_seg[c];
        if (k < 0 || k >= in->n_seg) return CSV_E_INVALID;
        const csv_segment& sg = in->seg[k];
        const int ch = sg.chrom;
        if (ch < 0 || ch >= in->n_chrom) return CSV_E_INVALID;
        const int aux = csv_soa::call_aux(R, c);
        o_seg[c] = k; o_aux[c] = aux; o_sup[c] = R.support[c]; o_cip[c] = csv_soa::cipos(R, c); o_cil[c] = csv_soa::cilen(R, c);
        o_dr[c] = csv_soa::dr(R, c); o_gl[c] = csv_soa::gl_idx(R, c);
        o_bp1[c] = csv_soa::bp1(R, c); o_bp2[c] = csv_soa::bp2(R, c);
        const bool gt_on = sg.genotype != 0 && o_gl[c] >= 0;
        if (gt_on) {                                                                    // (a filtered call's row is looked up too, as emit_slice does)
            const int32_t* it = std::lower_bound(in->gl_key, in->gl_key + in->n_gl, o_gl[c]);
            if (it == in->gl_key + in->n_gl || *it != o_gl[c] || !gl_ok[(size_t)(it - in->gl_key)]) return CSV_E_INVALID;
        }
        const int id = emitted_id(in, R, c);
        if (id < 0) continue;
        if (id == ID_INV) { if (aux < 0 || !in->strand_name || !in->strand_name[aux]) return CSV_E_INVALID; if (aux + 1 > n_strand) n_strand = aux + 1; }
        if (id == ID_BND && (aux < 0 || (aux >> 3) >= in->n_chrom)) return CSV_E_INVALID;
        if (in->genotype && gt_on && (o_sup[c] < 0 || o_dr[c] < 0 || (int64_t)o_sup[c] + o_dr[c] <= 0)) return CSV_E_INVALID;
        const int64_t slen = in->chrom_len ? in->chrom_len[ch] : 0;
        const RefRange rr = call_ref_range(in, R, c, slen);
        const bool readable = rr.e > rr.b && ref_range_inside(rr, slen);
        if (rr.e > rr.b && !readable && !rr.bnd) return CSV_E_INVALID;                   // a reference sequence is missing or too short
        if (ref_off[c] < 0 || ref_off[c + 1] - ref_off[c] != (readable ? rr.e - rr.b : 0)) return CSV_E_INVALID;
        o_ref[c] = ref_off[c]; o_ref[c + 1] = ref_off[c + 1];
        if (ref_off[c + 1] > ref_off[c] && !ref_blob) return CSV_E_INVALID;
        H.ref_bytes = std::max<vcf_i64>(H.ref_bytes, ref_off[c + 1]);
        if (with_alt && id == ID_INS) {
            if (in->ins_alt_off[c] < 0 || in->ins_alt_off[c + 1] < in->ins_alt_off[c]) return CSV_E_INVALID;
            H.alt_bytes = std::max<vcf_i64>(H.alt_bytes, in->ins_alt_off[c + 1]);
        }
        if (with_rn) {
            if (in->rnames_off[c] < 0 || in->rnames_off[c + 1] < in->rnames_off[c]) return CSV_E_INVALID;
            H.rn_bytes = std::max<vcf_i64>(H.rn_bytes, in->rnames_off[c + 1]);
        }
    }
    // (the offsets are read per call, c and c + 1: a call that was skipped above keeps its own pair out of the caller's arrays)
    for (int64_t c = 0; c <= nc; c++) { o_ref[c] = ref_off[c]; if (with_alt) o_alt[c] = in->ins_alt_off[c]; if (with_rn) o_rn[c] = in->rnames_off[c]; }
    std::vector<int32_t> seg3((size_t)in->n_seg * 3), chrom_off{0}, strand_off{0};
    for (int k = 0; k < in->n_seg; k++) { seg3[(size_t)k] = in->seg[k].svtype; seg3[(size_t)in->n_seg + k] = in->seg[k].chrom; seg3[(size_t)2 * in->n_seg + k] = in->seg[k].genotype; }
    std::vector<uint8_t> chrom, strand;
    std::vector<int64_t> chrom_len((size_t)in->n_chrom, 0);
    for (int i = 0; i < in->n_chrom; i++) {
        if (!in->chrom_name[i]) return CSV_E_INVALID;
        chrom.insert(chrom.end(), in->chrom_name[i], in->chrom_name[i] + strlen(in->chrom_name[i]));
        chrom_off.push_back((int32_t)chrom.size());
        if (in->chrom_len) chrom_len[(size_t)i] = in->chrom_len[i];
    }
    for (int i = 0; i < n_strand; i++) {
        const char* s = in->strand_name[i] ? in->strand_name[i] : "";
        strand.insert(strand.end(), s, s + strlen(s));
        strand_off.push_back((int32_t)strand.size());
    }
    // one block: every table at a multiple of 8
    struct Part { const void* p; size_t bytes; size_t at; };
    Part parts[] = {{c64.data(), c64.size() * 8, 0}, {chrom_len.data(), chrom_len.size() * 8, 0}, {c32.data(), c32.size() * 4, 0}, {seg3.data(), seg3.size() * 4, 0},
                    {chrom_off.data(), chrom_off.size() * 4, 0}, {strand_off.data(), strand_off.size() * 4, 0}, {in->gl_key, (size_t)in->n_gl * 4, 0}, {gl_off.data(), gl_off.size() * 4, 0},
                    {chrom.data(), chrom.size(), 0}, {strand.data(), strand.size(), 0}, {gl.data(), gl.size(), 0}, {gl_flag.data(), gl_flag.size(), 0}};
    size_t total = 0;
    for (Part& q : parts) { q.at = total; total += (q.bytes + 7) & ~(size_t)7; }
    H.pack.assign(total + 8, 0);
    for (const Part& q : parts) if (q.bytes) memcpy(H.pack.data() + q.at, q.p, q.bytes);
    char* b = H.pack.data();
    VcfView& V = H.view;
    V = VcfView{};
    V.n_calls = nc;
    const vcf_i64* p64 = (const vcf_i64*)(b + parts[0].at);
    V.bp1 = p64; V.bp2 = p64 + nc; V.ref_off = p64 + 2 * nc; V.alt_off = with_alt ? p64 + 3 * nc + 1 : nullptr; V.rn_off = with_rn ? p64 + 4 * nc + 2 : nullptr;
    V.chrom_len = (const vcf_i64*)(b + parts[1].at);
    const int32_t* p32 = (const int32_t*)(b + parts[2].at);
    V.call_seg = p32; V.call_aux = p32 + nc; V.support = p32 + 2 * nc; V.cipos = p32 + 3 * nc; V.cilen = p32 + 4 * nc; V.dr = p32 + 5 * nc; V.gl_idx = p32 + 6 * nc;
    const int32_t* ps = (const int32_t*)(b + parts[3].at);
    V.seg_type = ps; V.seg_chrom = ps + in->n_seg; V.seg_gt = ps + 2 * in->n_seg;
    V.n_chrom = in->n_chrom; V.chrom_off = (const int32_t*)(b + parts[4].at); V.chrom = (const uint8_t*)(b + parts[8].at);
    V.n_strand = n_strand; V.strand_off = (const int32_t*)(b + parts[5].at); V.strand = (const uint8_t*)(b + parts[9].at);
    V.n_gl = in->n_gl; V.gl_key = (const int32_t*)(b + parts[6].at); V.gl_off = (const int32_t*)(b + parts[7].at); V.gl = (const uint8_t*)(b + parts[10].at);
    V.gl_flag = (const uint8_t*)(b + parts[11].at);
    V.ref = (const uint8_t*)ref_blob; V.alt = (const uint8_t*)in->ins_alt; V.rn = (const uint8_t*)in->rnames;
    V.min_size = in->min_size; V.max_size = in->max_size; V.genotype = in->genotype; V.report_readid = in->report_readid; V.ignore_sequence = in->ignore_sequence;
    // emission order, as vcf_emit_impl makes it: a counting sort by chromosome, the chromosomes by rank, a stable sort by bp1 in each
    std::vector<int64_t> coff((size_t)in->n_chrom + 1, 0), idx((size_t)nc);
    for (int64_t c = 0; c < nc; c++) coff[(size_t)in->seg[R.call_seg[c]].chrom + 1]++;
    for (int i = 0; i < in->n_chrom; i++) coff[(size_t)i + 1] += coff[(size_t)i];
    {
        std::vector<int64_t> fill(coff.begin(), coff.end() - 1);
        for (int64_t c = 0; c < nc; c++) idx[(size_t)fill[(size_t)in->seg[R.call_seg[c]].chrom]++] = c;
    }
    std::vector<int> chroms(in->n_chrom);
    for (int i = 0; i < in->n_chrom; i++) chroms[i] = i;
    std::sort(chroms.begin(), chroms.end(), [&](int x, int y) { return in->chrom_rank[x] < in->chrom_rank[y]; });
    H.order.clear();
    H.order.reserve((size_t)nc);
    for (int ch : chroms) {
        std::stable_sort(idx.begin() + coff[(size_t)ch], idx.begin() + coff[(size_t)ch + 1], [&](int64_t x, int64_t y) { return o_bp1[x] < o_bp1[y]; });
        H.order.insert(H.order.end(), idx.begin() + coff[(size_t)ch], idx.begin() + coff[(size_t)ch + 1]);
    }
    return CSV_OK;
}

VcfView vcf_view_moved(const VcfHost& H, const char* base, const uint8_t* ref, const uint8_t* alt, const uint8_t* rn)
{
    VcfView V = H.view;
    const char* old = H.pack.data();
    auto mv = [&](auto*& p) { if (p) p = (std::remove_reference_t<decltype(p)>)(base + ((const char*)p - old)); };
    mv(V.call_seg); mv(V.call_aux); mv(V.support); mv(V.cipos); mv(V.cilen); mv(V.dr); mv(V.gl_idx); mv(V.bp1); mv(V.bp2); mv(V.ref_off); mv(V.alt_off); mv(V.rn_off);
    mv(V.seg_type); mv(V.seg_chrom); mv(V.seg_gt); mv(V.chrom_off); mv(V.chrom); mv(V.chrom_len); mv(V.strand_off); mv(V.strand); mv(V.gl_key); mv(V.gl_off); mv(V.gl); mv(V.gl_flag);
    V.ref = ref; V.alt = alt; V.rn = rn;
    return V;
}

}  // namespace csv

// csv_vcf_emit_ref's records from the record core with one lane and no context: the host form of csv_vcf_emit_device
extern "C" int csv_vcf_emit_core_host(const csv_vcf_in* in, const char* ref_blob, const int64_t* ref_off, char* out, int64_t cap, int64_t* n_written, int64_t* svid)
{
    if (!n_written || !svid) return CSV_E_INVALID;
    csv::VcfHost H;
    const int rc = csv::vcf_host_prepare(in, ref_blob, ref_off, H);
    if (rc != CSV_OK) return rc;
    const csv::VcfView& V = H.view;
    int64_t run[5] = {svid[0], svid[1], svid[2], svid[3], svid[4]}, total = 0;
    for (int64_t c : H.order) { const int id = csv::vcf_call_id(V, c); if (id >= 0) total += csv::vcf_record_len(V, c, id, run[id]++); }
    *n_written = total;
    if (!out || total > cap) return CSV_E_CAPACITY;
    int64_t at = 0, sv[5] = {svid[0], svid[1], svid[2], svid[3], svid[4]};
    for (int64_t c : H.order) { const int id = csv::vcf_call_id(V, c); if (id >= 0) at = csv::vcf_record_write(V, c, id, sv[id]++, (uint8_t*)out, at, 0, 1, nullptr); }
    for (int t = 0; t < 5; t++) svid[t] = run[t];
    return CSV_OK;
}

// ---------------------------------------------------------------------------------------- FASTA index
// The `.fai` of a FASTA file held in memory (mmap): per contig its name (up to the first white space of the header), length,
// byte offset of the first base, bases per line and bytes per line - what `samtools faidx` writes and pysam.FastaFile reads
// (generate_output opens the reference with it, cuteSV_genotype.py:254-259).  One memchr-driven pass; lines of a contig must
// have one length (the last may be shorter), like faidx demands.  Returns the number of contigs (may exceed max_contigs: call
// again with larger arrays), or -CSV_E_INVALID for a file that cannot be indexed.  name_off / name_len address the header text inside `data`.
extern "C" int64_t csv_fasta_index(const char* data, int64_t size, int64_t max_contigs, int64_t* name_off, int32_t* name_len,
                                   int64_t* length, int64_t* offset, int32_t* line_bases, int32_t* line_width)
{
    if (!data || size < 0) return -(int64_t)CSV_E_INVALID;
    int64_t n = 0, p = 0;
    while (p < size) {
        if (data[p] != '>') {                                       // (blank lines between records are tolerated)
            const char* nl = (const char*)memchr(data + p, '\n', (size_t)(size - p));
            if (!nl) break;
            if (nl != data + p && !(nl == data + p + 1 && data[p] == '\r')) return -(int64_t)CSV_E_INVALID;      // sequence before any header
            p = nl - data + 1;
            continue;
        }
        const char* nl = (const char*)memchr(data + p, '\n', (size_t)(size - p));
        const int64_t hdr_end = nl ? nl - data : size;
        int64_t e = p + 1;
        while (e < hdr_end && data[e] != ' ' && data[e] != '\t' && data[e] != '\r') e++;
        const int64_t seq0 = nl ? hdr_end + 1 : size;
        int64_t q = seq0, len = 0;
        int32_t lb = 0, lw = 0;
        bool last_short = false;
        while (q < size && data[q] != '>') {
            const char* l2 = (const char*)memchr(data + q, '\n', (size_t)(size - q));
            const int64_t le = l2 ? l2 - data : size;                  // end of the line's text
            int64_t bases = le - q;
            if (bases > 0 && data[le - 1] == '\r') bases--;
            const int64_t width = (l2 ? le + 1 : le) - q;
            if (bases == 0) { q = l2 ? le + 1 : size; last_short = true; continue; }      // an empty line ends the contig's regular part
            if (last_short) return -(int64_t)CSV_E_INVALID;                     // a longer line after a short one: not indexable
            if (lb == 0) { if (bases > INT32_MAX || width > INT32_MAX) return -(int64_t)CSV_E_INVALID; lb = (int32_t)bases; lw = (int32_t)width; }
            else if (bases > lb) return -(int64_t)CSV_E_INVALID;
            if (bases < lb || (l2 && width != lw)) last_short = true;
            len += bases;
            q = l2 ? le + 1 : size;
        }
        if (n < max_contigs) {
            if (name_off) name_off[n] = p + 1;
            if (name_len) name_len[n] = (int32_t)(e - (p + 1));
            if (length) length[n] = len;
            if (offset) offset[n] = seq0;
            if (line_bases) line_bases[n] = lb;
            if (line_width) line_width[n] = lw;
        }
        n++;
        p = q;
    }
    return n;
}

// ---------------------------------------------------------------------------------------- FASTA index, window after window
// csv_fasta_index for a text that is never in memory whole (a BGZF-compressed FASTA inflated window by window):
// for every cut of the text into windows, the entries and the verdict csv_fasta_index gives over the whole text.  The rules above are
// rules about whole lines - a line's first byte, its bytes, its last byte, whether a line break ends it - so the state between two
// windows is the line in progress (and, of a header line, its name so far).  The rules stand once more in ref_core.h's FaiStream,
// which also takes a window as event rows; tests/test_bgzf_reference.py holds it to csv_fasta_index at every cut.
struct csv_fai_stream : csv::FaiStream {};

extern "C" csv_fai_stream* csv_fasta_index_stream_open(void) { return new csv_fai_stream(); }
extern "C" void csv_fasta_index_stream_close(csv_fai_stream* s) { delete s; }

extern "C" int csv_fasta_index_stream_feed(csv_fai_stream* s, const char* data, int64_t size)
{
    if (!s || size < 0 || (size > 0 && !data)) return CSV_E_INVALID;
    return s->feed(data, size) ? CSV_OK : CSV_E_INVALID;
}

// The same window as event rows (ref_core.h: csv_fai_events' or csv_fai_events_host's): carry[3] <- what the next window's rows are
// made with; rows: 3 int64 per row; hdr: the header texts; tail[3]: the carry behind the window.  CSV_E_INVALID: the text is refused,
// or the rows do not describe a window behind the text fed so far.
extern "C" int csv_fasta_index_stream_carry(const csv_fai_stream* s, int64_t* carry)
{
    if (!s || !carry) return CSV_E_INVALID;
    const csv::FaiCarry c = s->carry();
    carry[0] = c.start; carry[1] = c.first; carry[2] = c.last;
    return CSV_OK;
}

extern "C" int csv_fasta_index_stream_rows(csv_fai_stream* s, const int64_t* rows, int64_t n_rows, const char* hdr, int64_t hdr_bytes, int64_t window_bytes, const int64_t* tail)
{
    if (!s || n_rows < 0 || hdr_bytes < 0 || window_bytes < 0 || !tail || (n_rows > 0 && !rows) || (hdr_bytes > 0 && !hdr)) return CSV_E_INVALID;
    static_assert(sizeof(csv::FaiRow) == 24, "a row is three int64");
    return s->rows((const csv::FaiRow*)rows, n_rows, hdr, hdr_bytes, window_bytes, csv::FaiCarry{tail[0], tail[1], tail[2]}) ? CSV_OK : CSV_E_INVALID;
}

// the end of the text: the last line, when no line break ended it, is judged now.  -> the number of contigs (the arrays hold the first
// max_contigs; *names_bytes = the bytes of all names, written back to back into names when they fit names_cap; name_off addresses
// them there), or -CSV_E_INVALID.  Call again with larger arrays when either is exceeded: finish may be repeated.
extern "C" int64_t csv_fasta_index_stream_finish(csv_fai_stream* s, int64_t max_contigs, char* names, int64_t names_cap, int64_t* names_bytes, int64_t* name_off,
                                                 int32_t* name_len, int64_t* length, int64_t* offset, int32_t* line_bases, int32_t* line_width)
{
    if (!s) return -(int64_t)CSV_E_INVALID;
    if (!s->finish()) return -(int64_t)CSV_E_INVALID;
    if (names_bytes) *names_bytes = (int64_t)s->names.size();
    if (names && (int64_t)s->names.size() <= names_cap) memcpy(names, s->names.data(), s->names.size());
    const int64_t n = (int64_t)s->ent.size();
    for (int64_t i = 0; i < n && i < max_contigs; i++) {
        const csv::FaiStream::Entry& e = s->ent[(size_t)i];
        if (name_off) name_off[i] = e.name_off;
        if (name_len) name_len[i] = e.name_len;
        if (length) length[i] = e.length;
        if (offset) offset[i] = e.offset;
        if (line_bases) line_bases[i] = e.lb;
        if (line_width) line_width[i] = e.lw;
    }
    return n;
}
