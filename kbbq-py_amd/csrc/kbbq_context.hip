// kbbq_context.hip -- libkbbq_hip.so (C ABI: include/kbbq_hip.h; gfx950 only): the context, device and page-locked memory, events,
// timing, the decoding of the status words -- and what every unit's entry points share (kbbq_lib.h): the error text, the
// argument checks, the context's scratch.
#include "kbbq_lib.h"
#include "bam_host.h"

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <string>

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

// for the host C++ files (kbbq_lib_host.h)
int kbbq_set_error_(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

static const u64 ST_INIT[KBBQ_NSTATUS] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};

// ---- launch helpers ---------------------------------------------------
int check_planes(const char* fn, int64_t nreads, int pitch, const void* a, const void* b, const void* c)
{
    if (nreads < 0) return fail(KBBQ_E_ARG, "%s: nreads < 0", fn);
    if (pitch <= 0 || (pitch & 15) || pitch > 65536) return fail(KBBQ_E_ARG, "%s: pitch must be a positive multiple of 16 (<= 65536), got %d", fn, pitch);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) return fail(KBBQ_E_ARG, "%s: planes must be 16-byte aligned", fn);
    return KBBQ_OK;
}

// errbit_ok: the call reads (or writes) KBBQ_ROWS_ERRBIT planes -- K1 / K2 on rows, the layout pass, the pair LUT; everything else that
// takes a 4-bit seq plane would read bit 3 as part of a code and refuses the flag
int layout_flags_ok(const char* who, int flags, bool errbit_ok)
{
    if (flags & ~(KBBQ_ROWS_PAIRS | KBBQ_ROWS_NIBBLES | KBBQ_ROWS_TWINS | KBBQ_ROWS_ERRBIT)) return fail(KBBQ_E_ARG, "%s: unknown layout flags 0x%x", who, flags);
    if (flags & KBBQ_ROWS_ERRBIT) {
        if (!errbit_ok) return fail(KBBQ_E_ARG, "%s: layout flags 0x%x: KBBQ_ROWS_ERRBIT planes are read by kbbq_accumulate_rows_dev / kbbq_apply_rows_dev only", who, flags);
        if ((flags & (KBBQ_ROWS_PAIRS | KBBQ_ROWS_NIBBLES)) != (KBBQ_ROWS_PAIRS | KBBQ_ROWS_NIBBLES))
            return fail(KBBQ_E_ARG, "%s: KBBQ_ROWS_ERRBIT describes 4-bit mate-pair rows (KBBQ_ROWS_PAIRS | KBBQ_ROWS_NIBBLES)", who);
    }
    if ((flags & KBBQ_ROWS_TWINS) && !(flags & KBBQ_ROWS_PAIRS)) return fail(KBBQ_E_ARG, "%s: KBBQ_ROWS_TWINS describes mate-pair rows (add KBBQ_ROWS_PAIRS)", who);
    return KBBQ_OK;
}

// context-owned device scratch of at least `need` bytes (contents are not kept).  The buffer it replaces may still be in use by
// what the stream holds: it is freed behind a synchronisation.
int grow_scratch(kbbq_ctx* c, DevScratch& s, size_t need)
{
    if (s.bytes >= need) return KBBQ_OK;
    if (s.p) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipFree(s.p); s.p = nullptr; s.bytes = 0; }
    HIPCHK(hipMalloc(&s.p, need));
    s.bytes = need;
    return KBBQ_OK;
}

// workgroups of a streaming kernel with a grid-stride loop: `per_cu` per CU.  Measured in three interleaved rounds (scripts/gpu_grids.sh,
// DESIGN.md section 6): 64 per CU -- four generations of workgroups per CU slot -- beat the 8-16 these kernels
// started with by 6-13 % (K4 1.95 -> 1.83 ms, K5 1.12 -> 0.98, K6 2.66 -> 2.37 per 16 M reads), 256 did for the layout pass
// (9.46 -> 8.42 ms per 50 M reads); one item per thread loses again where a workgroup has set-up work (K4's queue, K5's
// LDS counters and their flush: 13 ms).
int bounded_grid(int64_t want, const kbbq_ctx* c, int per_cu)
{
    const int64_t cap = (int64_t)c->cus * per_cu;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, cap));
}

extern "C" {

int kbbq_abi_version(void) { return KBBQ_ABI_VERSION; }
const char* kbbq_last_error(void) { return g_err.c_str(); }

int kbbq_device_count(int* count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(KBBQ_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return KBBQ_OK;
}

// host_affinity.cpp with the PCI address of HIP device `device`: a rank of a multi-GPU job binds its host threads to the
// NUMA node of ITS GPU (kbbq/parallel.py init_from_env, bench.py)
int kbbq_bind_host_to_device(int device, int* numa_node, int* ncpus)
{
    char busid[64] = {0};
    HIPCHK(hipDeviceGetPCIBusId(busid, (int)sizeof busid, device));
    return kbbq_bind_host_to_pci(busid, numa_node, ncpus);
}

int kbbq_ctx_create(int device, kbbq_ctx** out)
{
    if (!out) return fail(KBBQ_E_ARG, "kbbq_ctx_create: out is NULL");
    *out = nullptr;
    const bool dbg = getenv("KBBQ_CTX_DBG") != nullptr;         // where the context's first-use milliseconds go (stderr)
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[kbbq_ctx_create] %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    HIPCHK(hipSetDevice(device));
    lap("hipSetDevice");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    lap("hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(KBBQ_E_HIP, "libkbbq_hip is built for gfx950 only; device %d is %s", device, prop.gcnArchName);
    kbbq_ctx* c = new kbbq_ctx();
    c->device = device;
    c->cus = prop.multiProcessorCount;
    c->lds_bytes = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (c->lds_bytes <= 0) c->lds_bytes = 160 * 1024;
    snprintf(c->name, sizeof c->name, "%s (%s)", prop.name, prop.gcnArchName);
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(KBBQ_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    c->stream = c->own_stream;
    lap("hipStreamCreate");
    e = hipMalloc((void**)&c->d_status, sizeof ST_INIT);
    if (e != hipSuccess) { (void)hipStreamDestroy(c->own_stream); delete c; return fail(KBBQ_E_HIP, "hipMalloc(status): %s", hipGetErrorString(e)); }
    e = hipMemcpy(c->d_status, ST_INIT, sizeof ST_INIT, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(c->d_status); (void)hipStreamDestroy(c->own_stream); delete c; return fail(KBBQ_E_HIP, "hipMemcpy(status): %s", hipGetErrorString(e)); }
    lap("hipMalloc + hipMemcpy");
    // allow the full 160 KiB of LDS as dynamic shared memory to every kernel that is launched with dynamic LDS
    // (each unit for its own kernels, and a unit's first call loads ITS code object: a lap per unit)
    rows_full_lds(c->lds_bytes, lap);
    bgzf_full_lds(c->lds_bytes, lap);
    (void)hipGetLastError();
    *out = c;
    return KBBQ_OK;
}

int kbbq_ctx_destroy(kbbq_ctx* c)
{
    if (!c) return KBBQ_OK;
    (void)hipSetDevice(c->device);
    for (int w = 0; w < 2; ++w)
        for (auto& pr : c->ev[w]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->d_stats) (void)hipFree(c->d_stats);
    for (DevScratch* s : {&c->wgplan, &c->ops4, &c->tally, &c->rowlut, &c->bgzf_tok, &c->bgzf_off, &c->bgzf_blocks, &c->bam_words, &c->bam_index, &c->bam_recode})
        if (s->p) (void)hipFree(s->p);
    for (int b = 0; b < 2; ++b) {
        if (c->stage_host[b]) (void)hipHostFree(c->stage_host[b]);
        if (c->stage_dev[b]) (void)hipFree(c->stage_dev[b]);
        if (c->stage_up[b]) (void)hipEventDestroy(c->stage_up[b]);
        if (c->stage_used[b]) (void)hipEventDestroy(c->stage_used[b]);
        if (c->stage_down[b]) (void)hipEventDestroy(c->stage_down[b]);
    }
    kbbq_inflate_forget_ctx_(c);
    for (int b = 0; b < 2; ++b) {
        if (c->inflate_host[b]) (void)hipHostFree(c->inflate_host[b]);
        if (c->inflate_dev[b]) (void)hipFree(c->inflate_dev[b]);
        if (c->inflate_done[b]) (void)hipEventDestroy(c->inflate_done[b]);
    }
    if (c->inflate_stream) (void)hipStreamDestroy(c->inflate_stream);
    if (c->stage_stream) (void)hipStreamDestroy(c->stage_stream);
    if (c->stage_down_stream) (void)hipStreamDestroy(c->stage_down_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return KBBQ_OK;
}

int kbbq_ctx_set_stream(kbbq_ctx* c, void* s)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    c->stream = (hipStream_t)s;      // NULL is the device's default (null) stream, e.g. torch's
    return KBBQ_OK;
}

// for comm_rccl.cpp (not part of the public header)
void* kbbq_ctx_stream_(kbbq_ctx* c) { return c ? (void*)c->stream : nullptr; }
int kbbq_ctx_device_(kbbq_ctx* c) { return c ? c->device : 0; }

int kbbq_ctx_sync(kbbq_ctx* c)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_ctx_info(kbbq_ctx* c, int* cus, int* lds, char* name, int name_len)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (cus) *cus = c->cus;
    if (lds) *lds = c->lds_bytes;
    if (name && name_len > 0) { strncpy(name, c->name, (size_t)name_len - 1); name[name_len - 1] = 0; }
    return KBBQ_OK;
}

int kbbq_ctx_status(kbbq_ctx* c, int64_t* read_index)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    u64 st[KBBQ_NSTATUS];
    HIPCHK(hipMemcpyAsync(st, c->d_status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (read_index) *read_index = -1;
    if (st[0] == ~0ull && st[1] == ~0ull && st[2] == ~0ull && st[3] == ~0ull && st[ST_MEANQ] == ~0ull && st[ST_KMER] == ~0ull)
        return KBBQ_OK;
    HIPCHK(hipMemcpyAsync(c->d_status, ST_INIT, sizeof ST_INIT, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (st[ST_KMER] != ~0ull)
        return fail(KBBQ_E_FULL, "k-mer table full: an insert found no free slot within %d probes (give the table more slots)",
                    KM_MAX_PROBES);
    // the reference stops at the FIRST offending read; within one read the dinucleotide
    // lookup (TypeError, recalibrate.py:94) runs before the table indexing (IndexError, :114)
    if (st[0] == ~0ull && st[1] == ~0ull && st[2] == ~0ull && st[ST_MEANQ] != ~0ull) {
        if (read_index) *read_index = (int64_t)st[ST_MEANQ];
        return fail(KBBQ_E_MEANQ, "read group %lld: meanq lies on a truncation boundary (or the group has no counted base): "
                    "solve through kbbq_solve_dev with the host's longdouble meanq", (long long)st[ST_MEANQ]);
    }
    if (st[0] == ~0ull && st[1] == ~0ull && st[2] == ~0ull)
        return fail(KBBQ_E_LUT, "the device-built LUT can leave 0..255 or does not fit int8: re-run kbbq_apply_dev in checked mode");
    int code = KBBQ_E_TYPE; u64 best = st[ST_TYPE];
    if (st[ST_INDEX] < best) { best = st[ST_INDEX]; code = KBBQ_E_INDEX; }
    if (st[ST_RANGE] < best) { best = st[ST_RANGE]; code = KBBQ_E_RANGE; }
    if (read_index) *read_index = (int64_t)best;
    const char* what = code == KBBQ_E_TYPE ? "base outside ACGTN in a dinucleotide (reference: TypeError)"
                     : code == KBBQ_E_INDEX ? "quality/read-group/cycle beyond the tables (reference: IndexError)"
                                            : "recalibrated quality + 33 outside 0..255";
    return fail(code, "read %lld: %s", (long long)best, what);
}

int kbbq_dev_alloc(kbbq_ctx* c, size_t bytes, void** dptr)
{
    if (!c || !dptr) return fail(KBBQ_E_ARG, "kbbq_dev_alloc: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(dptr, bytes ? bytes : 16));
    return KBBQ_OK;
}

int kbbq_dev_free(kbbq_ctx* c, void* dptr)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (dptr) HIPCHK(hipFree(dptr));
    return KBBQ_OK;
}

int kbbq_dev_zero(kbbq_ctx* c, void* dptr, size_t bytes)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemsetAsync(dptr, 0, bytes, c->stream));
    return KBBQ_OK;
}

int kbbq_dev_upload(kbbq_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_dev_download(kbbq_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_dev_mem_info(kbbq_ctx* c, size_t* free_bytes, size_t* total_bytes)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return KBBQ_OK;
}

int kbbq_host_alloc(size_t bytes, void** hptr)
{
    if (!hptr) return fail(KBBQ_E_ARG, "kbbq_host_alloc: NULL argument");
    HIPCHK(hipHostMalloc(hptr, bytes ? bytes : 16, hipHostMallocDefault));
    return KBBQ_OK;
}

int kbbq_host_free(void* hptr)
{
    if (hptr) HIPCHK(hipHostFree(hptr));
    return KBBQ_OK;
}

int kbbq_dev_copy_async(kbbq_ctx* c, void* dst, const void* src, size_t bytes, int kind)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (kind < 1 || kind > 3) return fail(KBBQ_E_ARG, "kbbq_dev_copy_async: kind must be 1 (host to device), 2 (device to host) or 3 (device to device)");
    HIPCHK(hipSetDevice(c->device));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    return KBBQ_OK;
}

int kbbq_event_create(kbbq_ctx* c, void** ev)
{
    if (!c || !ev) return fail(KBBQ_E_ARG, "kbbq_event_create: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *ev = (void*)e;
    return KBBQ_OK;
}

int kbbq_event_record(kbbq_ctx* c, void* ev)
{
    if (!c || !ev) return fail(KBBQ_E_ARG, "kbbq_event_record: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord((hipEvent_t)ev, c->stream));
    return KBBQ_OK;
}

int kbbq_event_sync(void* ev)
{
    if (!ev) return fail(KBBQ_E_ARG, "kbbq_event_sync: NULL event");
    HIPCHK(hipEventSynchronize((hipEvent_t)ev));
    return KBBQ_OK;
}

int kbbq_event_destroy(void* ev)
{
    if (ev) HIPCHK(hipEventDestroy((hipEvent_t)ev));
    return KBBQ_OK;
}

size_t kbbq_tables_count(int R, int S2)
{
    return 2 * (size_t)R * KQ * (size_t)S2 + 2 * (size_t)R * KQ * KND;
}

int kbbq_ctx_timing(kbbq_ctx* c, int enable)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    c->timing = enable != 0;
    return KBBQ_OK;
}

int kbbq_ctx_kernel_ms(kbbq_ctx* c, int which, double* total_ms, int64_t* launches, int reset)
{
    if (!c || which < 0 || which > 1) return fail(KBBQ_E_ARG, "kbbq_ctx_kernel_ms: bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto& pr : c->ev[which]) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
        c->ms_acc[which] += ms;
        c->launches[which] += 1;
        (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
    }
    c->ev[which].clear();
    if (total_ms) *total_ms = c->ms_acc[which];
    if (launches) *launches = c->launches[which];
    if (reset) { c->ms_acc[which] = 0.0; c->launches[which] = 0; }
    return KBBQ_OK;
}

} // extern "C"
