// frame_core.h — BAM record framing in a window of inflated bytes, written once for the host and for the device (DESIGN.md
// section 29).  Plain C++: no HIP header, no global state.  The code is templated on a `Lanes` policy, as inflate_core.h is:
//   FrOneLane (below)       the host form: one lane.  It states the contract, it is what tests/frame_core_main.cpp runs under the
//                           address and undefined-behaviour sanitizers, and what the twin of the tests is.
//   FrWave (bam.hip.h)      the device form: the 64 lanes of a wavefront test 64 offsets at a time and share a CIGAR sum.
// What a Lanes type provides: lane(), width(), first(bool) (the lowest lane whose argument is true, -1: none; the same value in
// every lane), sum(int64) (the sum over the lanes, in every lane).
//
// W[0, n) is a window of the inflated stream, contiguous in stream order; the block table (off / len) says where its BGZF blocks
// lie in it; c is the offset of a known true record start.  The chain of true starts is serial: o -> o + 4 + block_size(o).
//   fr_guess    per block: the smallest offset that LOOKS like a record start (fr_plausible, three chain steps deep)
//   fr_chase    per block: the chain from an offset until it leaves the block -> the starts it met, and where it landed (`exit`)
//   fr_stitch   one lane: from c, block by block: a block whose guess IS the offset the true chain arrives at hands over its list
//               and its exit (the chain from an offset is deterministic: by induction from c every such list is the true chain's);
//               any other block is chased again from the true offset, serially.  The guess is a heuristic only: a wrong or
//               missed one costs one serial chase of one block and never changes the result.
//   fr_row      per framed record: the row the host's selection loop reads instead of the bytes
//   fr_layout   per selected record: where its parts go in the two images - the reader's emit branches, csv_frame_pack's range check
//
// Bounds, by construction.  The offsets are data-dependent and a false guess chases garbage, so every read compares its last
// byte with n first: fr_u32 is called only behind `o + 4 <= n` (block_size), `o + 36 <= n` (the fixed fields), `name_end <= n`
// (the name's last byte), `cigar word end <= record end <= n` (fr_row).  A chain step is taken only over a record that lies
// wholly inside the window with block_size >= 32: every step advances by at least 36 bytes, so every loop ends, a block's list
// holds at most len / 36 + 1 starts (its slot's size), and nothing is ever written outside a slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FRAME_FN __host__ __device__ inline
#else
#define FRAME_FN inline
#endif

namespace csv {

typedef long long fr_i64;

struct FrOneLane {
    FRAME_FN int lane() const { return 0; }
    FRAME_FN int width() const { return 1; }
    FRAME_FN int first(bool p) const { return p ? 0 : -1; }
    FRAME_FN fr_i64 sum(fr_i64 v) const { return v; }
};

struct FrWin { const uint8_t* w; fr_i64 n; int32_t n_ref; };

// one row per framed record: what the selection loop of the reader needs of it (40 bytes)
struct FrRow {
    fr_i64   off;           // the record's start (its block_size word) in the window
    fr_i64   span;          // sum over M / D / N / = / X of the record's own CIGAR words (the words inside the record)
    int32_t  block_size, refid, pos;
    uint32_t l_seq;
    uint16_t n_cigar;
    uint8_t  l_name, pad;
    uint32_t pad2;
};

// what the stitch found: tail = the start of the first record that is not wholly inside the window (n: the window ends on a
// record boundary); tail_bs = its block_size when those 4 bytes are inside (tail_has_bs), which may be < 32: the chain stops there
struct FrStitch { fr_i64 tail; int32_t tail_bs, tail_has_bs; fr_i64 n_records; int32_t right_blocks, fallback_blocks; };

// a selected record on its way into the images (k_frame_pack; host-checked: [src, src + 4 + bs) lies inside the window, the
// fields fit bs, the destinations lie inside the images)
struct FrPack { fr_i64 src, rec_off, host_off; int32_t bs; uint32_t l_seq; uint16_t n_cig; uint8_t l_name, pad; uint32_t pad2; };

// The layout of an emitted record.  Behind block_size a record holds 32 fixed bytes, the name, the CIGAR words, seq_bytes of bases,
// l_seq qualities, and the aux bytes from fixed_to_aux to bs (fixed_to_aux > bs: malformed, the caller checks).  Slim image: fixed
// bytes, CIGAR words, aux bytes = slim_len, zero padded to slim_padded (a slim record starts 16-byte aligned: its CIGAR words, at
// + 32, are too).  Host image: name and bases = host_len.  k_frame_pack (bam.hip.h) keeps its own statement of this formula.
struct FrLayout { fr_i64 seq_bytes, fixed_to_aux, slim_len, slim_padded, host_len; };
FRAME_FN FrLayout fr_layout(fr_i64 bs, fr_i64 l_name, fr_i64 n_cig, fr_i64 l_seq)
{
    FrLayout y;
    y.seq_bytes = (l_seq + 1) / 2; y.fixed_to_aux = 32 + l_name + 4 * n_cig + y.seq_bytes + l_seq;
    y.slim_len = 32 + 4 * n_cig + (bs - y.fixed_to_aux); y.slim_padded = (y.slim_len + 15) / 16 * 16;
    y.host_len = l_name + y.seq_bytes;
    return y;
}

constexpr fr_i64 FR_MAX_BS = 1ll << 28;
FRAME_FN fr_i64 fr_slot_size(fr_i64 block_len) { return block_len / 36 + 1; }

FRAME_FN uint32_t fr_u32(const uint8_t* w, fr_i64 o)          // (any alignment; the caller has compared o + 4 with n)
{
    return (uint32_t)w[o] | ((uint32_t)w[o + 1] << 8) | ((uint32_t)w[o + 2] << 16) | ((uint32_t)w[o + 3] << 24);
}

// one record's plausibility at o: 1 = passes, 0 = fails, -1 = it cannot be read inside the window (fixed fields or the name's
// last byte lie beyond n).  *next: where its chain step leads (set when it passes)
FRAME_FN int fr_plausible1(const FrWin& W, fr_i64 o, fr_i64* next)
{
    if (o < 0 || o + 36 > W.n) return -1;
    const fr_i64 bs = (fr_i64)fr_u32(W.w, o);
    if (bs < 32 || bs >= FR_MAX_BS) return 0;
    const int32_t refid = (int32_t)fr_u32(W.w, o + 4), next_refid = (int32_t)fr_u32(W.w, o + 24);
    if (refid < -1 || refid >= W.n_ref || next_refid < -1 || next_refid >= W.n_ref) return 0;
    const fr_i64 l_name = W.w[o + 12];
    if (l_name < 1) return 0;
    const fr_i64 n_cig = (fr_i64)(fr_u32(W.w, o + 16) & 0xffffu), l_seq = (fr_i64)fr_u32(W.w, o + 20);
    if (32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs) return 0;
    if (o + 36 + l_name > W.n) return -1;
    if (W.w[o + 36 + l_name - 1] != 0) return 0;
    *next = o + 4 + bs;
    return 1;
}

// the test of a guess: the record at o passes, and the next two chain steps pass or leave the window
FRAME_FN bool fr_plausible(const FrWin& W, fr_i64 o)
{
    fr_i64 nx = 0;
    if (fr_plausible1(W, o, &nx) != 1) return false;
    for (int step = 0; step < 2; step++) {
        const int r = fr_plausible1(W, nx, &nx);
        if (r == 0) return false;
        if (r < 0) return true;
    }
    return true;
}

// the smallest offset in [beg, end) that passes fr_plausible; -1: none.  width() offsets per round; every lane gets the result
template <class L> FRAME_FN fr_i64 fr_guess(const L& ln, const FrWin& W, fr_i64 beg, fr_i64 end)
{
    for (fr_i64 base = beg; base < end; base += ln.width()) {
        const fr_i64 o = base + ln.lane();
        const int f = ln.first(o < end && fr_plausible(W, o));
        if (f >= 0) return base + f;
    }
    return -1;
}

// the chain from o (inside the block that ends at blk_end) until it leaves the block: the starts go to slot[0 .. *count), at
// most fr_slot_size(block length) of them.  -> exit: where the chain landed - the first start at or beyond blk_end, or the
// start of a record that is not wholly inside the window or has block_size < 32 (the chain cannot step over it)
FRAME_FN fr_i64 fr_chase(const FrWin& W, fr_i64 o, fr_i64 blk_end, fr_i64* slot, fr_i64 slot_cap, int32_t* count)
{
    int32_t k = 0;
    while (o < blk_end) {
        if (o + 4 > W.n) break;
        const fr_i64 bs = (fr_i64)(int32_t)fr_u32(W.w, o);
        if (bs < 32 || o + 4 + bs > W.n) break;
        if (k >= slot_cap) break;                                // (cannot happen: 36 bytes a step; the slot is never overrun whatever the arithmetic)
        slot[k++] = o;
        o += 4 + bs;
    }
    *count = k;
    return o;
}

// From c to the window's end.  g / ex / cnt: the guess, the exit and the list length of every block (fr_guess, fr_chase);
// slot_off[s]: where block s's slot starts in `starts`.  used[s] becomes the number of starts of block s that are the true
// chain's (0 for a block the chain never lands in: its list is never consulted).
FRAME_FN void fr_stitch(const FrWin& W, int32_t n_blocks, const fr_i64* blk_off, const int32_t* blk_len, const fr_i64* slot_off, const fr_i64* g, const fr_i64* ex,
                        const int32_t* cnt, fr_i64* starts, int32_t* used, fr_i64 c, FrStitch* out)
{
    FrStitch R;
    R.tail = W.n; R.tail_bs = 0; R.tail_has_bs = 0; R.n_records = 0; R.right_blocks = 0; R.fallback_blocks = 0;
    for (int32_t s = 0; s < n_blocks; s++) used[s] = 0;
    fr_i64 t = c;
    int32_t s = 0;
    for (;;) {
        R.tail = t; R.tail_has_bs = 0;
        if (t < 0 || t + 4 > W.n) break;
        const fr_i64 bs = (fr_i64)(int32_t)fr_u32(W.w, t);
        R.tail_bs = (int32_t)bs; R.tail_has_bs = 1;
        if (bs < 32 || t + 4 + bs > W.n) break;
        while (s < n_blocks && blk_off[s] + blk_len[s] <= t) s++;
        if (s >= n_blocks || blk_off[s] > t) break;              // (t lies in no block of the table: a table with a gap - nothing is framed there)
        if (g[s] == t) { used[s] = cnt[s]; t = ex[s]; R.right_blocks++; }
        else {
            int32_t k = 0;
            t = fr_chase(W, t, blk_off[s] + blk_len[s], starts + slot_off[s], fr_slot_size(blk_len[s]), &k);
            used[s] = k; R.fallback_blocks++;
        }
        R.n_records += used[s];
    }
    *out = R;
}

// the row of the record at o, which lies wholly inside the window with block_size >= 32 (fr_chase stepped over it); lane 0's
// copy is complete.  The CIGAR words are read only inside the record, whatever n_cigar says.
template <class L> FRAME_FN FrRow fr_row(const L& ln, const FrWin& W, fr_i64 o)
{
    FrRow r;
    r.off = o;
    r.block_size = (int32_t)fr_u32(W.w, o);
    r.refid = (int32_t)fr_u32(W.w, o + 4); r.pos = (int32_t)fr_u32(W.w, o + 8);
    r.l_name = W.w[o + 12];
    r.n_cigar = (uint16_t)(fr_u32(W.w, o + 16) & 0xffffu);
    r.l_seq = fr_u32(W.w, o + 20);
    r.pad = 0; r.pad2 = 0;
    const fr_i64 rec_end = o + 4 + (fr_i64)r.block_size, cg = o + 36 + (fr_i64)r.l_name;
    fr_i64 n_in = cg <= rec_end ? (rec_end - cg) / 4 : 0;
    if (n_in > (fr_i64)r.n_cigar) n_in = (fr_i64)r.n_cigar;
    fr_i64 span = 0;
    for (fr_i64 k = ln.lane(); k < n_in; k += ln.width()) {
        const uint32_t w = fr_u32(W.w, cg + 4 * k), op = w & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += (fr_i64)(w >> 4);
    }
    r.span = ln.sum(span);
    return r;
}

}  // namespace csv

// ---- The reader's way to the device (stage_frame.hip.h), for bam_host.cpp alone: inside the library, not part of the C ABI.
// A window is loaded (csv_frame_window: the kept tail moves to the front of the other buffer, the new blocks are inflated behind
// it; csv_frame_window_put: a block the host had to inflate), framed from a cursor (csv_frame_run: the rows and the stitch's
// verdict come down, nothing else), and the records the reader selects are packed into the device images (csv_frame_chunk_begin,
// csv_frame_pack per window, csv_frame_chunk_end).  `owner` names the reader whose chunk the context holds.
struct csv_ctx;
#define FRAME_LOCAL extern "C" __attribute__((visibility("hidden")))
FRAME_LOCAL int csv_frame_window(csv_ctx* c, const uint8_t* comp, int64_t comp_bytes, int32_t n_blocks, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                                 const int32_t* out_len, const uint32_t* crc, int64_t bytes, int64_t keep, int64_t keep_at, uint8_t* status, double* ms_kernels);
FRAME_LOCAL uint64_t csv_frame_window_serial(const csv_ctx* c);          // counts the windows loaded: a reader whose number is not the last does not own the window
FRAME_LOCAL int csv_frame_window_put(csv_ctx* c, int64_t off, const uint8_t* src, int64_t len);
FRAME_LOCAL int csv_frame_run(csv_ctx* c, int32_t n_blocks, const int64_t* blk_off, const int32_t* blk_len, int32_t n_ref, int64_t cursor, const csv::FrRow** rows, csv::FrStitch* res);
FRAME_LOCAL int csv_frame_chunk_begin(csv_ctx* c, const void* owner);
FRAME_LOCAL int csv_frame_pack(csv_ctx* c, int64_t n, const csv::FrPack* p, int64_t slim_bytes, int64_t host_bytes);
FRAME_LOCAL int csv_frame_chunk_end(csv_ctx* c, int64_t n, const int64_t* rec_off, const uint32_t* rec_len, const int64_t* host_off, const int32_t* l_name, const int32_t* l_seq);
FRAME_LOCAL int csv_frame_reader(csv_ctx* c, const void* owner, int set);      // set: `owner` becomes the context's one framing reader (CSV_E_STATE: it has another); else: it leaves, its chunk dies
FRAME_LOCAL int csv_frame_fetch(csv_ctx* c, const void* owner, uint8_t* slim, uint8_t* host);
FRAME_LOCAL int csv_frame_counters(csv_ctx* c, int64_t* right, int64_t* fallback, double* ms_kernels, int64_t* bytes_down, int64_t* bytes_up, int reset);
