// cutesv_hip.hip — libcutesv_hip.so's one translation unit.  This file: the pinned-range registry, the ABI / device / host-memory
// entries, context create / destroy / sync and two measurement aids.  ctx.hip.h: the context, the state struct of every stage and
// the shared helpers.  stage_upload / stage_run / stage_results.hip.h: the cluster engine of include/cutesv_hip.h (upload, run,
// validate, download, publish).  The other stage_*.hip.h (included last): the extraction stages.  gfx950 only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "wave.hip.h"
#include "scan.hip.h"
#include "kernels.hip.h"
#include "sort.hip.h"
#include "cigar.hip.h"
#include "split.hip.h"
#include "bam.hip.h"
#include "sa.hip.h"
#include "names.hip.h"
#include "seqs.hip.h"
#include "vcf_strings.hip.h"
#include "aln.hip.h"
#include "gates.hip.h"
#include "reads.hip.h"

using namespace csv;

namespace {

// Page-locked host ranges handed out (or registered) through this library, process wide: {base -> bytes, device address}.
// csv_batch_download writes results straight into such memory from a kernel; a range leaves the table before it is freed,
// so a table hit is always live memory (addresses pinned by other means are asked about through the HIP runtime each time).
struct PinnedRange { size_t bytes; char* dev; bool owned; };
std::mutex g_pinned_mu;
std::map<uintptr_t, PinnedRange> g_pinned;
void pinned_note(void* p, size_t bytes, bool owned)
{
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned[(uintptr_t)p] = PinnedRange{bytes, (char*)d, owned};
}
void pinned_forget(void* p)
{
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned.erase((uintptr_t)p);
}
// device address of host pointer p (with `bytes` behind it) if it is page-locked, else nullptr.  Memory from csv_host_alloc
// is owned by this library (it leaves the table in csv_host_free, before it is released): a hit there is live memory.  A
// range the CALLER registered (csv_host_register) may have been freed or re-used without csv_host_unregister - a kernel
// writing through such a stale mapping would fault the GPU - so those hits, like unknown addresses, are confirmed with
// the HIP runtime on every use.
void* pinned_device_address(const void* p, size_t bytes)
{
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        auto it = g_pinned.upper_bound((uintptr_t)p);
        if (it != g_pinned.begin()) {
            --it;
            const uintptr_t off = (uintptr_t)p - it->first;
            if (off < it->second.bytes) {
                if (off + bytes > it->second.bytes) return nullptr;
                if (it->second.owned) return it->second.dev + off;
            }
        }
    }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    if (bytes > 1) {                                            // the last byte must belong to the same page-locked range
        hipPointerAttribute_t a2;
        if (hipPointerGetAttributes(&a2, (const char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (a2.type != hipMemoryTypeHost || (char*)a2.devicePointer != (char*)at.devicePointer + bytes - 1) return nullptr;
    }
    return at.devicePointer;
}

// one timing slot per launch (group), in launch order
const char* kStageName[CSV_N_STAGES] = {"init", "k_chain_count", "k_chain_apply", "k_refine_indel_wave", "k_refine_wave", "k_refine_mid",
                                        "k_refine_block", "k_items_scan", "k_emit", "k_reads_order", "k_reads_gather", "k_reads_maxlen",
                                        "k_genotype", "k_genotype_tra", "event_floor", "", "", "", "", "", "", "", "", ""};
constexpr int N_COPY_STREAMS = 2;
constexpr int RO_CAP = 4096;                 // sorted runs the reads_order stage plans (k_reads_plan packs the rank in 12 bits)

}  // namespace

#include "ctx.hip.h"

// the engine: host code of upload, run and delivery, one file per stage
#include "stage_upload.hip.h"
#include "stage_run.hip.h"
#include "stage_results.hip.h"

extern "C" {

int csv_abi_version(void) { return CSV_ABI_VERSION; }

int csv_struct_size(int which)
{
    switch (which) {
    case 0: return (int)sizeof(csv_segment);
    case 1: return (int)sizeof(csv_batch_in);
    case 2: return (int)sizeof(csv_batch_out);
    case 3: return (int)sizeof(csv_run_stats);
    case 4: return (int)sizeof(csv_rebuild_in);
    case 5: return (int)sizeof(csv_rebuild_out);
    case 6: return (int)sizeof(csv_vcf_in);
    case 7: return (int)sizeof(csv_rows_in);
    case 8: return (int)sizeof(csv_cigar_in);
    case 9: return (int)sizeof(csv_cigar_out);
    case 10: return (int)sizeof(csv_split_in);
    case 11: return (int)sizeof(csv_split_out);
    default: return -1;
    }
}

const char* csv_stage_name(int s) { return (s >= 0 && s < CSV_N_STAGES) ? kStageName[s] : ""; }

int csv_device_count(int* n)
{
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (n) *n = (e == hipSuccess) ? k : 0;
    return e == hipSuccess ? CSV_OK : CSV_E_HIP;
}

int csv_device_info(int device_id, char* pci_bus_id, int cap, int* n_cu)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return CSV_E_HIP;
    if (pci_bus_id && cap > 0) { pci_bus_id[0] = 0; if (hipDeviceGetPCIBusId(pci_bus_id, cap, device_id) != hipSuccess) return CSV_E_HIP; }
    if (n_cu && hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess) return CSV_E_HIP;
    return CSV_OK;
}

int32_t csv_gl_index(int64_t c0, int64_t c1)
{
    if (c0 == 3 && c1 == 1) return 101 * 101;
    if (c0 == 6 && c1 == 2) return 101 * 101 + 1;
    const int64_t total = c0 + c1;
    if (total > 100) {
        const double frac = (double)c0 / (double)total;
        c0 = (int64_t)(100.0 * frac);
        c1 = 100 - c0;
    }
    return (int32_t)(c0 * 101 + c1);
}

int csv_host_alloc(int64_t bytes, void** out)
{
    if (!out || bytes < 0) return CSV_E_INVALID;
    *out = nullptr;
    void* p = nullptr;
    const size_t n = (size_t)(bytes > 0 ? bytes : 1);
    if (hipHostMalloc(&p, n, hipHostMallocPortable) != hipSuccess) return CSV_E_NOMEM;
    pinned_note(p, n, true);
    *out = p;
    return CSV_OK;
}
void csv_host_free(void* p) { if (p) { pinned_forget(p); (void)hipHostFree(p); } }
int csv_host_register(void* p, int64_t bytes)
{
    if (!p || bytes <= 0) return CSV_E_INVALID;
    if (hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable) != hipSuccess) return CSV_E_HIP;
    pinned_note(p, (size_t)bytes, false);
    return CSV_OK;
}
int csv_host_unregister(void* p) { if (p) pinned_forget(p); return (p && hipHostUnregister(p) == hipSuccess) ? CSV_OK : CSV_E_HIP; }

int csv_ctx_create(int device_id, csv_ctx** out)
{
    if (!out) return CSV_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return CSV_E_HIP;
    csv_ctx* c = new csv_ctx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) { delete c; return CSV_E_HIP; }
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || c->n_cu < 1) c->n_cu = 256;
    for (auto& e : c->ev) if (hipEventCreate(&e) != hipSuccess) { delete c; return CSV_E_HIP; }
    {
        // side[2] carries the reads stage, whose critical path runs through two single-workgroup kernels (k_reads_plan,
        // k_pmax_scan): at default priority they wait for a free CU behind the clustering kernels of the main stream
        // (27 and 15 us in the trace for a few microseconds of work), so that stream gets the highest priority
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        for (int q = 0; q < 3; q++) {
            const hipError_t e = (q == 2 && !getenv("CSV_NO_PRIORITY")) ? hipStreamCreateWithPriority(&c->side[q], hipStreamNonBlocking, greatest)
                                                                          : hipStreamCreateWithFlags(&c->side[q], hipStreamNonBlocking);
            if (e != hipSuccess) { delete c; return CSV_E_HIP; }
        }
    }
    for (auto& s2 : c->copy) if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) { delete c; return CSV_E_HIP; }
    if (hipStreamCreateWithFlags(&c->res.pub, hipStreamNonBlocking) != hipSuccess) { delete c; return CSV_E_HIP; }
    for (int q = 0; q < 2; q++)
        if (hipEventCreateWithFlags(&c->res.ev_run[q], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->res.ev_pub[q], hipEventDisableTiming) != hipSuccess) { delete c; return CSV_E_HIP; }
    if (hipEventCreateWithFlags(&c->ev_init, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_sel, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_reads, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_anc, hipEventDisableTiming) != hipSuccess) { delete c; return CSV_E_HIP; }
    for (auto& e : c->ev_aux) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete c; return CSV_E_HIP; }
    for (auto& e : c->ev_rd) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete c; return CSV_E_HIP; }
    for (auto& e : c->ev_copy) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete c; return CSV_E_HIP; }
    {
        void* hf = nullptr;
        if (hipHostMalloc(&hf, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
            void* df = nullptr;
            if (hipHostGetDevicePointer(&df, hf, 0) == hipSuccess) { c->h_flag = (volatile int*)hf; c->d_flag = (int*)df; memset(hf, 0, 64); }
            else (void)hipHostFree(hf);
        }
    }
    if (reserve(c, c->res.cnt, 1024) || reserve(c, c->ro.rstate, sizeof(ReadsState)) || pin_reserve(c, 1 << 20) || sqrt_table(c, SQRT_TAB)) {
        delete c;
        return CSV_E_HIP;
    }
    *out = c;
    return CSV_OK;
}

void csv_ctx_destroy(csv_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    std::vector<Buf*> own = {&c->flush};
    c->ro.own(own); c->res.own(own); c->tab.own(own);
    c->pool.own(own); c->sp.own(own); c->bm.own(own); c->sa.own(own); c->nm.own(own); c->seq.own(own); c->vs.own(own); c->al.own(own); c->rt.own(own); c->inf.own(own); c->fr.own(own); c->ixb.own(own); c->dfl.own(own); c->ref.own(own); c->ve.own(own); c->bs.own(own); c->sam.own(own);
    for (Buf* b : own) if (b->p) (void)hipFree(b->p);
    for (Arena* a : {&c->arena, &c->scratch, &c->bm.arena, &c->sa.arena, &c->nm.arena}) if (a->base) (void)hipFree(a->base);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    if (c->h_flag) (void)hipHostFree((void*)c->h_flag);
    if (c->res.h_pub) (void)hipHostFree(c->res.h_pub);
    for (auto& ps : c->res.pub_stage) if (ps) (void)hipFree(ps);
    for (int q = 0; q < 2; q++) { if (c->res.ev_run[q]) (void)hipEventDestroy(c->res.ev_run[q]); if (c->res.ev_pub[q]) (void)hipEventDestroy(c->res.ev_pub[q]); }
    if (c->res.pub) (void)hipStreamDestroy(c->res.pub);
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_aux) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_copy) if (e) (void)hipEventDestroy(e);
    if (c->ev_init) (void)hipEventDestroy(c->ev_init);
    if (c->ev_sel) (void)hipEventDestroy(c->ev_sel);
    if (c->ev_reads) (void)hipEventDestroy(c->ev_reads);
    if (c->ev_anc) (void)hipEventDestroy(c->ev_anc);
    for (auto& e : c->ev_rd) if (e) (void)hipEventDestroy(e);
    for (auto& s2 : c->side) if (s2) (void)hipStreamDestroy(s2);
    for (auto& s2 : c->copy) if (s2) (void)hipStreamDestroy(s2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* csv_last_error(const csv_ctx* c) { return c ? c->err.c_str() : "null context"; }

int csv_ctx_sync(csv_ctx* c)
{
    if (!c) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CSV_OK;
}

int csv_measure_copy_bandwidth(csv_ctx* c, int64_t bytes, int reps, double* gb_per_s)
{
    if (!c || !gb_per_s || bytes <= 0 || reps <= 0) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    void *src = nullptr, *dst = nullptr;
    if (hipMalloc(&src, (size_t)bytes) != hipSuccess || hipMalloc(&dst, (size_t)bytes) != hipSuccess) {
        if (src) (void)hipFree(src);
        return fail(c, CSV_E_NOMEM, "copy-bandwidth buffers (%lld bytes each)", (long long)bytes);
    }
    (void)hipMemsetAsync(src, 1, (size_t)bytes, c->stream);
    float best = 1e30f;
    hipError_t e = hipSuccess;
    for (int r = 0; r < reps && e == hipSuccess; r++) {
        e = hipEventRecord(c->ev[0], c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev[1], c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(c->ev[1]);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
        if (e == hipSuccess && ms < best) best = ms;
    }
    (void)hipFree(src); (void)hipFree(dst);
    if (e != hipSuccess) return fail(c, CSV_E_HIP, "copy-bandwidth measurement: %s", hipGetErrorString(e));
    *gb_per_s = 2.0 * (double)bytes / ((double)best * 1e-3) / 1e9;
    return CSV_OK;
}

int csv_cache_flush(csv_ctx* c, int64_t bytes)
{
    if (!c || bytes <= 0) return CSV_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = reserve(c, c->flush, (size_t)bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(c->flush.p, 0x5a, (size_t)bytes, c->stream));
    return CSV_OK;
}

}  // extern "C"

// the extraction-side stages: host code over the kernel headers above, one file per stage
#include "stage_pool.hip.h"
#include "stage_names.hip.h"
#include "stage_seqs.hip.h"
#include "stage_rebuild.hip.h"
#include "stage_vcf_strings.hip.h"
#include "stage_sigs_text.hip.h"
#include "stage_extract.hip.h"
#include "stage_bam.hip.h"
#include "stage_inflate.hip.h"
#include "stage_deflate.hip.h"
#include "stage_vcf_emit.hip.h"
#include "stage_ref.hip.h"
#include "stage_frame.hip.h"
#include "stage_index.hip.h"
#include "stage_bam_sort.hip.h"
#include "stage_sam.hip.h"
#include "stage_aln.hip.h"
#include "stage_gates.hip.h"
#include "stage_reads.hip.h"
