// gates.hip.h — the gates of an extraction task on the columns csv_bam_decode left on the device.
//
// Restates extract._gates: single_pipe's gates (cuteSV main script :711 secondary records, :725 a read belongs to the task it
// starts in, :715-723 --include_bed) and parse_read's own (:607 query length, :614 MAPQ), one byte of CSV_GATE_* bits per record.
//
//   k_task_gates    one thread per record, grid-stride: five loads, at most one search of the region table, one byte store
//
// --include_bed without a loop over the regions.  The reference asks whether SOME region of the task's list has
// end > b0 and start < b1.  With the list sorted by b0 (load_bed sorts it), the regions with b0 < end are a prefix of length k,
// found by halving; one of them has b1 > start exactly when the largest b1 of the prefix has.  pmax_end[j] = max(b1 of regions
// 0 .. j) is made on the host and uploaded beside the table.  This holds for any regions: nested (a long early region covers a
// read that the last region in front of it does not), overlapping, with negative starts or with b1 < b0.
//
// The table is read from global memory: the records of a chunk are sorted by start, so the searches of a wavefront walk
// the same few cache lines.  No LDS, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.hip.h"

namespace csv {

constexpr int GATE_TASK = 1, GATE_PARSED = 2, GATE_USE = 4, GATE_SEL = 8, GATE_READS = 16;

struct GateArgs {
    i64 n;                          // records of the decoded chunk
    const i64* ref_start; const i64* ref_end; const int* mapq; const int* qlen; const uint8_t* cls; const i64* sa_off;
    i64 task_start;
    int min_read_len, min_mapq;
    int bed;                        // CSV_GT_BED: a record must overlap a region
    i64 n_regions;
    const i64* beg;                 // n_regions, non-decreasing
    const i64* pmax_end;            // n_regions: running maximum of the regions' ends
    uint8_t* bits;                  // n
};

__global__ __launch_bounds__(256) void k_task_gates(GateArgs A)
{
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < A.n; i += stride) {
        const i64 s = A.ref_start[i];
        const int cls = A.cls[i];
        bool task = cls != 0 && s >= A.task_start;
        if (task && A.bed) {
            const i64 e = A.ref_end[i];
            i64 lo = 0, hi = A.n_regions;            // partition point: the regions [0, lo) have beg < e
            while (lo < hi) {
                const i64 mid = lo + ((hi - lo) >> 1);
                if (A.beg[mid] < e) lo = mid + 1; else hi = mid;
            }
            task = lo > 0 && A.pmax_end[lo - 1] > s;
        }
        int b = 0;
        if (task) {
            const int mq = A.mapq[i] >= A.min_mapq;
            b = GATE_TASK | (mq ? GATE_READS : 0);
            if (A.qlen[i] >= A.min_read_len) {
                b |= GATE_PARSED | (mq ? GATE_USE : 0);
                if (cls == 1 && A.sa_off[i + 1] > A.sa_off[i]) b |= GATE_SEL;
            }
        }
        A.bits[i] = (uint8_t)b;
    }
}

}  // namespace csv
