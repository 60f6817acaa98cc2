// reads.hip.h — the genotyping reads table in device memory.
//
// The reads table of the reference (cuteSV main script :729-733) holds one row per record that passed the task gates with
// mapq >= min_mapq: (reference_start, reference_end, is_primary, name).  Every column of it exists on the device when a task's
// chunk is decoded - BamState.start / end / cls, the gates byte (CSV_GATE_READS), the name pool's index - so the table is cut out
// of them here and never travels:
//   start    ref_start (BAM positions are int32: pos is an int32_t field of the record, so the cast loses nothing)
//   end      ref_end, saturating at INT32_MAX as in the alignment table (pos + span of a record near 2^31 - 1)
//   primary  cls == 1 (flag 0 or 16)
//   id       name_base + the record's index in its chunk: the name pool's index of its name
// one row per kept record, grouped by chromosome, in append order (inside an append: record order).
//
//   k_reads_keep    one thread per decoded record: cnt = {flag byte & mask != 0, 0, 0, 0}; the flag bytes are the gates column
//                   (mask = CSV_GATE_READS) or the caller's keep bytes (mask = 0xff); the exclusive scan is
//                   scan.hip.h's (scan_counts: k_scan_tiles / k_scan_offsets)
//   k_reads_store   one thread per decoded record: the kept ones become rows behind the table's last row (four stores); the
//                   thread of the last kept record also leaves its id - the largest of the append - in last_id
//   k_reads_put     the same for rows that came from host arrays
//   k_reads_rank    one thread per row: out[i] = rank[id[i]], the gather through NameState.rank (ids are host-checked against
//                   the name pool's row count)
// The rows are written behind the committed count and become part of the table when the host moves the count after the call
// succeeded: a refused append changes nothing a later call reads (the alignment table's rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"

namespace csv {

constexpr int READS_INT_MAX = 0x7fffffff;

struct ReadsCols { int* start; int* end; uint8_t* primary; int* id; };

__global__ __launch_bounds__(256) void k_reads_keep(const uint8_t* flags, int mask, i64 n, int4* cnt)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cnt[i] = make_int4((flags[i] & mask) ? 1 : 0, 0, 0, 0);
}

// cnt holds the exclusive offsets, n_keep the number of kept records (the host has read it: n_keep > 0)
__global__ __launch_bounds__(256) void k_reads_store(ReadsCols T, i64 n0, const i64* pos, const i64* ref_end, const uint8_t* cls, const uint8_t* flags, int mask, i64 n,
                                                     int name_base, const int4* cnt, i64 n_keep, int* last_id)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !(flags[i] & mask)) return;
    const i64 k = cnt[i].x;
    if (k < 0 || k >= n_keep) return;                                   // (cannot happen: the offsets are the scan of the same bytes)
    const i64 r = n0 + k, e = ref_end[i];
    const int id = name_base + (int)i;
    T.start[r] = (int)pos[i];
    T.end[r] = e > READS_INT_MAX ? READS_INT_MAX : (int)e;
    T.primary[r] = cls[i] == 1 ? 1 : 0;
    T.id[r] = id;
    if (k == n_keep - 1) *last_id = id;
}

__global__ __launch_bounds__(256) void k_reads_put(ReadsCols T, i64 n0, const int* start, const int* end, const uint8_t* primary, const int* id, i64 n)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T.start[n0 + i] = start[i];
    T.end[n0 + i] = end[i];
    T.primary[n0 + i] = primary[i] ? 1 : 0;
    T.id[n0 + i] = id[i];
}

__global__ __launch_bounds__(256) void k_reads_rank(const int* id, const int* rank, int* out, i64 n)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rank[id[i]];
}

}  // namespace csv
