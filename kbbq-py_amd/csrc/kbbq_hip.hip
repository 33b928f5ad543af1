// kbbq_hip.hip -- C ABI of libkbbq_hip.so (see include/kbbq_hip.h).
// gfx950 only.  Host side: launch geometry, device staging, status decoding.
// K1 / K2 launch through one layer: the kernel tables (K1_VARIANTS, LDS_KERNELS) and launch_lds; K1's LDS geometry is k1_geometry +
// k1_lds_plan + launch_k1, K2's choice between persistent and short-lived workgroups k2_tile_serves; k2v3_params / k2t_params /
// fill_row_lut / k4_params fill the parameter structs, grow_scratch grows the context's device scratch.
#include "kbbq_kernels.h"
#include "kbbq_kernels_v3.h"
#include "kbbq_k2_tile.h"
#include "kbbq_solve_kernels.h"
#include "kbbq_lut_kernels.h"
#include "kbbq_aligned_kernels.h"
#include "kbbq_layout_kernels.h"
#include "kbbq_apply_aligned.h"
#include "kbbq_kmer.h"
#include "kbbq_kmer_set.h"
#include "kbbq_bgzf.h"
#include "kbbq_bam_out.h"
#include "kbbq_bam_index.h"
#include "kbbq_bgzf_inflate.h"
#include "bam_host.h"
#include "../../include/kbbq_hip.h"
#include "host_threads.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

// an environment switch that a test or bench.py sets: is it `value`?
static bool env_is(const char* name, const char* value) { const char* v = getenv(name); return v && !strcmp(v, value); }

// used by fastq_host.cpp
int kbbq_set_error_(int code, const char* msg) { g_err = msg ? msg : ""; return code; }

#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(KBBQ_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                           \
    } while (0)

struct DevScratch { void* p = nullptr; size_t bytes = 0; };

struct kbbq_ctx {
    int device = 0;
    int cus = 0;
    int lds_bytes = 0;
    char name[128] = {0};
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    u64* d_status = nullptr;          // [KBBQ_NSTATUS]
    int* d_stats = nullptr;           // [K7_NSTATS] scratch of kbbq_meta_stats_dev
    // device scratch of the context's own, grown on demand (grow_scratch)
    DevScratch wgplan;                // K2 (short-lived workgroups): first workgroup of every read group
    DevScratch ops4;                  // K4: one 32-byte record of the first CIGAR operations per read
    DevScratch tally;                 // kbbq_tally_aligned_dev: [count | flags words of the reads | rows K4 still has to look at]
    DevScratch rowlut;                // K2 on one-read-per-row planes: the LUT narrowed to the rows' pitch
    DevScratch bgzf_tok;              // kbbq_bgzf_deflate*: the tokens of the blocks in flight (a workgroup's worth each)
    DevScratch bgzf_off;              // ... the blocks' offsets in the packed output, and its length
    DevScratch bgzf_blocks;           // kbbq_bgzf_deflate (host buffers): a slab's blocks before they are packed
    DevScratch bam_words;             // kbbq_bam_assemble_dev: the lowest row with a quality below 0, the lowest that does not fit
    DevScratch bam_index;             // kbbq_bam_index_dev: words, keys, runs, lengths, head rows, workgroup totals (csrc/kbbq_bam_index.h)
    // kbbq_inflate_bgzf: staging and a stream of its own -- a reader may inflate on a thread of its own while the context's other
    // staging is in use -- and the lock that makes it one call at a time
    void* inflate_host[2] = {nullptr, nullptr}; void* inflate_dev[2] = {nullptr, nullptr}; size_t inflate_bytes = 0;
    hipStream_t inflate_stream = nullptr;
    hipEvent_t inflate_done[2] = {nullptr, nullptr};
    std::mutex inflate_lock;
    // host-buffer entry points (stage_run): two page-locked staging slabs and their device twins, a copy stream and
    // the events that order host copy -> upload -> kernel -> download slab by slab (grown on demand, kept for the next call)
    void* stage_host[2] = {nullptr, nullptr}; void* stage_dev[2] = {nullptr, nullptr}; size_t stage_bytes = 0;
    hipStream_t stage_stream = nullptr;      // uploads
    hipStream_t stage_down_stream = nullptr; // downloads (kbbq_apply): a stream of their own, so that slab k + 1 goes up while slab k comes back
    hipEvent_t stage_up[2] = {nullptr, nullptr}, stage_used[2] = {nullptr, nullptr}, stage_down[2] = {nullptr, nullptr};
    bool timing = false;
    // per-kernel event pairs recorded while timing is on
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];
    double ms_acc[2] = {0.0, 0.0};
    int64_t launches[2] = {0, 0};
};

#define KBBQ_NSTATUS 8

// Tuned launch constants (measured in earlier rounds: DESIGN.md, profiles/)
constexpr size_t K2T_ROW_LUT_MAX = 52 << 10;  // short-lived K2 on one-read-per-row planes: a read group's LUT of up to 52 KB
constexpr int K2V3_FRONTS = 8;               // sequential fronts of the persistent K2 traversal (K2v3Params::parts)
constexpr int K2T_XCD_TILES = 1;             // short-lived K2: every XCD walks a contiguous eighth of the planes (K2tParams::xcd_tiles)
constexpr int K2T_XCD = 8;                   // k2t_order: the read groups' workgroups of one position on the same XCD
constexpr int K7_FRONTS = 8;                 // sequential fronts of k7_lay_out (LayOutParams::parts)
constexpr int TALLY_K4_SHARE = 8;            // kbbq_tally_aligned_dev: K4's grid is sized for 1 / 8 of the reads
static const u64 ST_INIT[KBBQ_NSTATUS] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};

// ---- kernels launched with dynamic LDS ---------------------------------------------------------------------------------
// Each of them is named HERE and nowhere else: launch_lds takes a kernel's address from these tables, and kbbq_ctx_create walks the
// same tables to allow every one of them the full LDS as dynamic shared memory.  An instance that is not listed is not
// instantiated and cannot be selected.
// K1 (table-driven): form x copies of the context table (DN) x 4-bit planes (NIB) x chunk-position-major cycle table of KJ chunks
// x the error flag in bit 3 of the seq nibbles (EB, KBBQ_ROWS_ERRBIT: the KJ forms only), each without and with SPLIT (a dinucleotide
// threshold above the counting one)
enum K1Form { K1_ROWS, K1_ALIGNED, K1_ALIGNED_REF, K1_BANDS };
struct K1Variant { K1Form form; int dn, nib, kj, eb; const void* kernel[2]; };   // kernel[split]
#define K1_SPLITS(K, ...) {(const void*)(K<false, __VA_ARGS__>), (const void*)(K<true, __VA_ARGS__>)}
static const K1Variant K1_VARIANTS[] = {
    {K1_ROWS, K1V3_DNREP, 0, 0, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP)},
    {K1_ROWS, 8, 0, 0, 0, K1_SPLITS(k1v3_accumulate, 8)},
    {K1_ROWS, K1V3_DNREP, 1, 0, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true)},
    {K1_ROWS, 8, 1, 0, 0, K1_SPLITS(k1v3_accumulate, 8, true)},
    {K1_ROWS, K1V3_DNREP, 1, 13, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 13)},
    {K1_ROWS, K1V3_DNREP, 1, 19, 0, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 19)},
    {K1_ROWS, K1V3_DNREP, 1, 13, 1, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 13, true)},
    {K1_ROWS, K1V3_DNREP, 1, 19, 1, K1_SPLITS(k1v3_accumulate, K1V3_DNREP, true, 19, true)},
    {K1_ALIGNED, K1V3_DNREP, 0, 0, 0, K1_SPLITS(k1v3_aligned, K1V3_DNREP)},
    {K1_ALIGNED, 8, 0, 0, 0, K1_SPLITS(k1v3_aligned, 8)},
    {K1_ALIGNED_REF, K1V3_DNREP, 0, 0, 0, K1_SPLITS(k1v3_aligned_ref, K1V3_DNREP)},
    {K1_ALIGNED_REF, 8, 0, 0, 0, K1_SPLITS(k1v3_aligned_ref, 8)},
    {K1_BANDS, 0, 0, 0, 0, K1_SPLITS(k1v3_bands, false)},                          // every band brings its own DN (K1BandsParams::dn)
    {K1_BANDS, 0, 1, 0, 0, K1_SPLITS(k1v3_bands, true)},
};
#undef K1_SPLITS

static const void* k1_kernel(K1Form form, bool split, int dn, int nib, int kj, int eb = 0)
{
    for (const K1Variant& v : K1_VARIANTS)
        if (v.form == form && v.dn == dn && v.nib == nib && v.kj == kj && v.eb == eb) return v.kernel[split];
    return nullptr;                                                             // launch_lds reports it
}

// the others: the round-1 kernels (tables beyond the LDS, KBBQ_APPLY_CHECKED) and K2
enum LdsKernel { LK_K1_PLAIN, LK_K1_PLAIN_SPLIT, LK_K1_TILED, LK_K1_TILED_SPLIT, LK_K2V3, LK_K2V3_NIB, LK_K2V3_NIB_EB, LK_K2T, LK_K2T_NIB, LK_K2T_BANDS, LK_K2T_PAIR19, LK_K2T_PAIR13, LK_K2T_PAIR19_EB, LK_K2T_PAIR13_EB, LK_K2_LDS16, LK_K2_LDS8, LK_BGZF, LK_BGZF_INFLATE, LK_COUNT };
static const void* const LDS_KERNELS[LK_COUNT] = {
    (const void*)k1_accumulate<false>, (const void*)k1_accumulate<true>,
    (const void*)k1_accumulate_tiled<false>, (const void*)k1_accumulate_tiled<true>,
    (const void*)k2v3_apply<false>, (const void*)k2v3_apply<true>, (const void*)k2v3_apply<true, true>,
    (const void*)k2t_apply<false>, (const void*)k2t_apply<true>, (const void*)k2t_bands,
    (const void*)k2t_apply_pair<19>, (const void*)k2t_apply_pair<13>, (const void*)k2t_apply_pair<19, true>, (const void*)k2t_apply_pair<13, true>,
    (const void*)k2_apply<int16_t, true, true>, (const void*)k2_apply<int8_t, true, false>,
    (const void*)bz_deflate, (const void*)bi_inflate,
};

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
    // (the first call loads the code object: KBBQ_CTX_DBG shows it apart)
    auto full_lds = [&](const void* kernel) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, c->lds_bytes);
        if (kernel == LDS_KERNELS[0]) lap("first hipFuncSetAttribute");
    };
    for (const void* kernel : LDS_KERNELS) full_lds(kernel);
    for (const K1Variant& v : K1_VARIANTS) { full_lds(v.kernel[0]); full_lds(v.kernel[1]); }
    (void)hipGetLastError();
    lap("the other attributes");
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
    for (DevScratch* s : {&c->wgplan, &c->ops4, &c->tally, &c->rowlut, &c->bgzf_tok, &c->bgzf_off, &c->bgzf_blocks, &c->bam_words, &c->bam_index})
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

int kbbq_lut_row_stride(int S2) { return lut_row_stride(S2); }

static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t lut_full_offset(int R, int Qt, int S2) { return align16((size_t)R * Qt * lut_row_stride(S2) * 2); }
size_t kbbq_full_lut_bytes(int R, int Qt, int S2) { return (size_t)R * (33 + Qt) * (size_t)full_lut_row_bytes(S2); }
static size_t lut_compact8_offset(int R, int Qt, int S2) { return lut_full_offset(R, Qt, S2) + align16(kbbq_full_lut_bytes(R, Qt, S2)); }
static size_t lut_compact8_bytes(int R, int Qt, int S2) { return (size_t)R * Qt * lut_row_stride(S2); }
static size_t lut_flags_offset(int R, int Qt, int S2) { return lut_compact8_offset(R, Qt, S2) + align16(lut_compact8_bytes(R, Qt, S2)); }
size_t kbbq_lut_bytes(int R, int Qt, int S2) { return lut_flags_offset(R, Qt, S2) + 16; }

size_t kbbq_lut_count(int R, int Qt, int S2)
{
    return (size_t)R * Qt * (size_t)lut_row_stride(S2);     // even: K2 stages the LUT as 32-bit words
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

// ---- launch helpers ---------------------------------------------------
static int check_planes(const char* fn, int64_t nreads, int pitch, const void* a, const void* b, const void* c)
{
    if (nreads < 0) return fail(KBBQ_E_ARG, "%s: nreads < 0", fn);
    if (pitch <= 0 || (pitch & 15) || pitch > 65536) return fail(KBBQ_E_ARG, "%s: pitch must be a positive multiple of 16 (<= 65536), got %d", fn, pitch);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) return fail(KBBQ_E_ARG, "%s: planes must be 16-byte aligned", fn);
    return KBBQ_OK;
}

static u32 magic_for(int cpr) { return cpr <= 1 ? 0u : (u32)(((1ull << 32) + (u64)cpr - 1) / (u64)cpr); }

struct Timed {
    kbbq_ctx* c; int which; hipEvent_t a = nullptr, b = nullptr;
    Timed(kbbq_ctx* c_, int w) : c(c_), which(w)
    {
        if (c->timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
            (void)hipEventRecord(a, c->stream);
        else a = b = nullptr;
    }
    ~Timed()
    {
        if (a && b) { (void)hipEventRecord(b, c->stream); c->ev[which].push_back({a, b}); }
    }
};

// the one launch of a kernel with dynamic LDS: `kernel` comes from K1_VARIANTS (k1_kernel) or LDS_KERNELS, all of which take one
// parameter struct; `which`: the timer the launch counts for (kbbq_ctx_kernel_ms: 0 = K1, 1 = K2)
static int launch_lds(kbbq_ctx* c, int which, const void* kernel, dim3 grid, dim3 block, size_t lds, const void* params)
{
    if (!kernel) return fail(KBBQ_E_HIP, "libkbbq_hip has no instance of K1 for this launch (K1_VARIANTS)");
    void* args[] = {const_cast<void*>(params)};
    {
        Timed t(c, which);
        (void)hipLaunchKernel(kernel, grid, block, args, lds, c->stream);
    }
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// context-owned device scratch of at least `need` bytes (contents are not kept).  The buffer it replaces may still be in use by
// what the stream holds: it is freed behind a synchronisation.
static int grow_scratch(kbbq_ctx* c, DevScratch& s, size_t need)
{
    if (s.bytes >= need) return KBBQ_OK;
    if (s.p) { HIPCHK(hipStreamSynchronize(c->stream)); (void)hipFree(s.p); s.p = nullptr; s.bytes = 0; }
    HIPCHK(hipMalloc(&s.p, need));
    s.bytes = need;
    return KBBQ_OK;
}

extern "C" {

int kbbq_accumulate_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq,
                        const uint8_t* d_qual, const uint32_t* d_meta,
                        int64_t nreads, int pitch, int R, int S2, int minscore, int64_t* d_tables)
{
    return kbbq_accumulate_ex_dev(c, d_seq, d_cseq, d_qual, d_meta, nreads, pitch, R, S2,
                                  minscore, minscore, d_tables);
}

// what accumulate_rows would launch (kernel parameters, LDS bytes, template variant): kbbq_accumulate_bands_dev collects
// these for all length bands and launches them as ONE kernel
struct K1Setup { K1v3Params q; int dn = 0; int kj = 0; int eb = 0; size_t lds = 0; };    // dn / kj / eb: K1_VARIANTS; lds: bytes of dynamic LDS
static int accumulate_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                           const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2, int minscore,
                           int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables, bool* fits, int S_band = 0, int S_min = 0, int nib = 0,
                           int twins = 0, K1Setup* setup_only = nullptr, int errbit = 0);

int kbbq_accumulate_ex_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq,
                           const uint8_t* d_qual, const uint32_t* d_meta,
                           int64_t nreads, int pitch, int R, int S2, int minscore,
                           int dinuc_minscore, int64_t* d_tables)
{
    return kbbq_accumulate_band_dev(c, d_seq, d_cseq, d_qual, d_meta, nreads, pitch, R, S2, 0, 0, minscore, dinuc_minscore, d_tables);
}

int kbbq_accumulate_band_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq,
                             const uint8_t* d_qual, const uint32_t* d_meta,
                             int64_t nreads, int pitch, int R, int S2, int S_band, int S_min, int minscore,
                             int dinuc_minscore, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_accumulate_dev", nreads, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (R <= 0 || R > 32767) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: R out of range (%d)", R);
    if (S2 <= 0 || (S2 & 1)) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: S2 must be positive and even (%d)", S2);
    if (minscore < 0 || minscore > KQ - 1) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: minscore out of range (%d)", minscore);
    if (dinuc_minscore < 0 || dinuc_minscore > 222) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: dinuc_minscore out of range (%d)", dinuc_minscore);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));

    const int64_t nblocks = (nreads + 63) / 64;
    const bool split = dinuc_minscore > minscore;
    bool fits = false;
    rc = accumulate_rows(c, "kbbq_accumulate_dev", d_seq, d_cseq, d_qual, d_meta, nreads, pitch, 0, R, S2, minscore,
                         dinuc_minscore, nullptr, d_tables, &fits, S_band, S_min);
    if (rc || fits) return rc;                          // launched (or a real error); otherwise the tables do not fit the LDS
    K1Params p;
    p.seq = d_seq; p.cseq = d_cseq; p.qual = d_qual; p.meta = d_meta;
    p.nreads = nreads; p.pitch = pitch; p.cpr = pitch / 16; p.cpr_magic = magic_for(p.cpr);
    p.R = R; p.S2 = S2; p.minscore = dinuc_minscore;   // the TypeError rule follows the dinucleotide threshold
    p.qlo = 33u + (u32)minscore; p.dlo = 33u + (u32)dinuc_minscore;
    p.pos_stride = S2 | 1;                         // odd row stride spreads q rows over the banks
    p.tables = reinterpret_cast<u64*>(d_tables); p.status = c->d_status;
    auto lds_of = [](int stride) { return ((size_t)(((KQ * stride) + 1) & ~1)) * 4 + (size_t)KQ * KND * 8; };
    size_t lds = lds_of(p.pos_stride);
    K1TiledParams tp;
    int tiles = 1;
    if (lds > (size_t)c->lds_bytes) {
        // the KQ x S2 table is beyond the LDS: the fewest equal tiles of an even number of columns whose KQ x (tile_w | 1) table fits
        const int max_w = (int)((((size_t)c->lds_bytes - (size_t)KQ * KND * 8) / 4 - 1) / KQ - 1) & ~1;
        if (max_w < 2) return fail(KBBQ_E_ARG, "kbbq_accumulate_dev: %d B of LDS hold no tile of the tables", c->lds_bytes);
        tiles = (S2 + max_w - 1) / max_w;
        tp.tile_w = ((S2 + tiles - 1) / tiles + 1) & ~1;
        tiles = (S2 + tp.tile_w - 1) / tp.tile_w;
        p.pos_stride = tp.tile_w | 1;
        lds = lds_of(p.pos_stride);
    }
    int per_cu = std::min<int>((int)(c->lds_bytes / lds), 2048 / K1_THREADS);
    per_cu = std::max(per_cu, 1);
    if (tiles > 1) {                                // k1_accumulate_tiled: a workgroup iteration is K1_THREADS chunks
        tp.k = p;
        const int64_t iters = (nreads * p.cpr + K1_THREADS - 1) / K1_THREADS;
        const int gx = (int)std::min<int64_t>(iters, std::max<int64_t>(1, (int64_t)c->cus * per_cu / ((int64_t)R * tiles)));
        return launch_lds(c, 0, LDS_KERNELS[split ? LK_K1_TILED_SPLIT : LK_K1_TILED], dim3((unsigned)gx, (unsigned)R, (unsigned)tiles),
                          dim3(K1_THREADS), lds, &tp);
    }
    const int64_t iters = (nblocks + (K1_THREADS / 64) - 1) / (K1_THREADS / 64);
    int gx = (int)std::min<int64_t>(iters, std::max(1, c->cus * per_cu / R));
    return launch_lds(c, 0, LDS_KERNELS[split ? LK_K1_PLAIN_SPLIT : LK_K1_PLAIN], dim3((unsigned)gx, (unsigned)R, 1), dim3(K1_THREADS), lds, &p);
}

// host twin of k3_fill_full_lut (same rules; the GPU test compares the two blobs byte for byte)
static int fill_full_lut_host(const int16_t* lut16, int rs16, int R, int Qt, int S2, int minscore, int8_t* full,
                              int8_t* compact8)
{
    const int rb = full_lut_row_bytes(S2);
    const int NR = 33 + Qt;
    int bad = 0;
    for (int r = 0; r < R; ++r)
        for (int qb = 0; qb < NR; ++qb) {
            int8_t* row = full + ((size_t)r * NR + qb) * rb;
            for (int x = 0; x < rb; ++x) {
                const int W = full_lut_width(S2);
                int v = 0;
                if (qb < 33 + minscore) { if (x < 2 * W) v = qb == 0 ? -33 : qb - 33; }
                else {
                    const int16_t* src = lut16 + ((size_t)r * Qt + (qb - 33)) * rs16;
                    if (x < S2) v = src[x];
                    else if (x >= W && x < W + S2) v = src[S2 - 1 - (x - W)];
                    else if (x >= 2 * W && x < 2 * W + 25) v = src[S2 + (x - 2 * W)];
                }
                if (v < -128 || v > 127) bad |= 1;
                row[x] = (int8_t)v;
            }
        }
    for (size_t i = 0; i < (size_t)R * Qt * rs16; ++i) {
        if (lut16[i] < -128 || lut16[i] > 127) bad |= 1;
        compact8[i] = (int8_t)lut16[i];
    }
    for (int r = 0; r < R; ++r)
        for (int q = minscore; q < Qt; ++q) {
            const int16_t* src = lut16 + ((size_t)r * Qt + q) * rs16;
            int lo1 = 32767, hi1 = -32768, lo2 = 32767, hi2 = -32768;
            for (int x = 0; x < S2; ++x) { lo1 = std::min<int>(lo1, src[x]); hi1 = std::max<int>(hi1, src[x]); }
            for (int x = 0; x < 25; ++x) { lo2 = std::min<int>(lo2, src[S2 + x]); hi2 = std::max<int>(hi2, src[S2 + x]); }
            if (lo1 + lo2 + 33 < 0 || hi1 + hi2 + 33 > 255) bad |= 2;
        }
    return bad;
}

int kbbq_build_lut(int R, int Qt, int S2, int D, int minscore, const int64_t* meanq, const int64_t* rgdq,
                   const int64_t* qdq, const int64_t* posdq, const int64_t* dinucdq, void* blob,
                   int* flags_out)
{
    // D = 17 is what get_delta_qs returns (applybqsr.py:98-101); D = 16 is accepted because the
    // reference's own apply test passes an unpadded table (index -1 then aliases column 15)
    if (R <= 0 || Qt <= 0 || Qt > 95 || S2 <= 0 || D < 16 || D > 17 || minscore < 0)
        return fail(KBBQ_E_ARG, "kbbq_build_lut: bad shape R=%d Qt=%d S2=%d D=%d minscore=%d", R, Qt, S2, D, minscore);
    memset(blob, 0, kbbq_lut_bytes(R, Qt, S2));
    int16_t* out = reinterpret_cast<int16_t*>(blob);
    const int rs = lut_row_stride(S2);
    for (int r = 0; r < R; ++r)
        for (int q = 0; q < Qt; ++q) {
            const size_t cell = (size_t)r * Qt + q;
            int16_t* row = out + cell * rs;
            const int64_t base = meanq[r] + rgdq[r] + qdq[cell];
            for (int s = 0; s < S2; ++s) {
                const int64_t v = base + posdq[cell * S2 + s];
                if (v < -32768 || v > 32767) return fail(KBBQ_E_RANGE, "kbbq_build_lut: value %lld does not fit the LUT", (long long)v);
                row[s] = (int16_t)v;
            }
            // dinucleotide index 5 * prev + cur, codes A0 T1 G2 C3 and 4 = N / no previous base;
            // anything involving code 4 is the reference's index -1, i.e. column D - 1
            for (int a = 0; a < 5; ++a)
                for (int b = 0; b < 5; ++b) {
                    const int64_t v = (a < 4 && b < 4) ? dinucdq[cell * D + 4 * a + b] : dinucdq[cell * D + (D - 1)];
                    if (v < -32768 || v > 32767) return fail(KBBQ_E_RANGE, "kbbq_build_lut: value %lld does not fit the LUT", (long long)v);
                    row[S2 + 5 * a + b] = (int16_t)v;
                }
        }
    int8_t* full = reinterpret_cast<int8_t*>(blob) + lut_full_offset(R, Qt, S2);
    int8_t* compact8 = reinterpret_cast<int8_t*>(blob) + lut_compact8_offset(R, Qt, S2);
    const int flags = fill_full_lut_host(out, rs, R, Qt, S2, std::min(minscore, Qt), full, compact8);
    *reinterpret_cast<int*>(reinterpret_cast<char*>(blob) + lut_flags_offset(R, Qt, S2)) = flags;
    if (flags_out) *flags_out = flags;
    return KBBQ_OK;
}

// K2 on one-read-per-row planes of this pitch: the cycle width Sb of the LUT, the columns such rows can reach
// (KBBQ_K2_ROWLUT=0: the tables' full S2, A/B timing)
static int row_lut_width(int pitch, int S2) { return env_is("KBBQ_K2_ROWLUT", "0") ? S2 : std::min(pitch, S2); }

// the LUT of cycle width Sb (k3_fill_row_lut) written to `dst`, on the launch stream in front of the apply kernel that reads it
static const int8_t* fill_row_lut(kbbq_ctx* c, const void* d_lut_blob, int R, int Qt, int S2, int Sb, int minscore, void* dst)
{
    RowLutParams f;
    f.lut16 = reinterpret_cast<const int16_t*>(d_lut_blob); f.rs16 = lut_row_stride(S2); f.R = R; f.Qt = Qt; f.S2 = S2; f.Sb = Sb;
    f.minscore = std::min(std::max(minscore, 0), Qt);
    f.out = reinterpret_cast<int8_t*>(dst);
    hipLaunchKernelGGL(k3_fill_row_lut, dim3((unsigned)(R * (33 + Qt))), dim3(256), 0, c->stream, f);
    return f.out;
}

// ... when Sb < S2, that narrowed LUT in context-owned scratch (Sb == S2: the blob's own full LUT is used, *lut untouched).
// False: no scratch for it.
static bool narrowed_row_lut(kbbq_ctx* c, const void* d_lut_blob, int R, int Qt, int S2, int Sb, int minscore, const int8_t** lut)
{
    if (Sb >= S2) return true;
    if (grow_scratch(c, c->rowlut, (size_t)R * (33 + Qt) * full_lut_row_bytes(Sb))) return false;
    *lut = fill_row_lut(c, d_lut_blob, R, Qt, S2, Sb, minscore, c->rowlut.p);
    return true;
}

// Does K2 run with short-lived workgroups (kbbq_k2_tile.h) on rows of `cpr` chunks, `rg_bytes` of LUT per read group?  Mate-pair
// rows and one-read-per-row planes, 4-bit and character planes (round 4; KBBQ_K2_TILE_CHARS=0: the persistent kernel as before),
// one read group or rows grouped by read group, unless KBBQ_K2_TILE=0 (A/B timing); everything else, and LUTs of one group beyond
// a third of the LDS, keeps the persistent kernel
// (one read per row: while two workgroups' copies of the narrowed LUT fit a CU -- rows of up to ~300 bases; measured up to
//  there, scripts/gpu_tilekb.sh: config 5's K2 0.651 -> 0.687 of roofline going from a 32 KB to a 52 KB limit)
static bool k2_tile_serves(const kbbq_ctx* c, int pairs, int nib, int R, bool grouped, int cpr, size_t rg_bytes)
{
    if (env_is("KBBQ_K2_TILE", "0") || (!nib && env_is("KBBQ_K2_TILE_CHARS", "0"))) return false;
    if ((R != 1 && !grouped) || cpr < 2 || cpr > 4096) return false;
    return pairs ? rg_bytes * 3 <= (size_t)c->lds_bytes : rg_bytes <= K2T_ROW_LUT_MAX;
}

// K2v3Params of rows whose LUT has Qt quality rows and, one read per row, the cycle width Sb (mate-pair rows: their own LUT,
// d_pair_lut).  q.full is the blob's full LUT: the caller narrows it (narrowed_row_lut, fill_row_lut) when Sb < S2.
static K2v3Params k2v3_params(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows, int pitch,
                              int pairs, int R, int Qt, int S2, int Sb, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                              const int64_t* d_seg, const int64_t* d_perm, uint8_t* d_out)
{
    K2v3Params q;
    q.seq = d_seq; q.qual = d_qual; q.meta = d_meta; q.nreads = nrows; q.pitch = pitch;
    q.cpr = pitch / 16; q.cpr_magic = magic_for(q.cpr);
    q.R = R; q.Qt = Qt; q.S2 = S2; q.minscore = minscore; q.qlo = 33u + (u32)minscore;
    q.lut16 = reinterpret_cast<const int16_t*>(d_lut_blob); q.rs16 = lut_row_stride(S2);
    q.full = pairs ? reinterpret_cast<const int8_t*>(d_pair_lut)
                   : reinterpret_cast<const int8_t*>(d_lut_blob) + lut_full_offset(R, Qt, S2);
    q.rb = (u32)(pairs ? pair_lut_row_bytes(S2) : full_lut_row_bytes(Sb));
    q.full_bytes = (int)((size_t)R * (33 + Qt) * q.rb);
    if (pairs) { q.W = 0u; q.ctx_off = (u32)pair_pitch(S2); q.maxlen = S2 + 1; }
    else { q.W = (u32)full_lut_width(Sb); q.ctx_off = 2u * q.W; q.maxlen = Sb; }
    q.pairs = pairs; q.seg = reinterpret_cast<const long long*>(d_seg);
    q.perm = reinterpret_cast<const long long*>(d_perm);
    q.parts = K2V3_FRONTS;
    q.rpb = 64;      // the persistent kernel's wave block; smaller blocks were measured slower (profiles/r01_traversal_microbench.md)
    q.out = d_out; q.status = c->d_status;
    return q;
}

// the persistent K2 on these rows: every read group's LUT in the LDS, or -- rows grouped by read group -- a slice of the grid
// per group with that group's
static int launch_k2v3(kbbq_ctx* c, const K2v3Params& q, int nib, int errbit = 0)
{
    const int slices = q.seg ? q.R : 1;
    const size_t lds = (size_t)(33 + q.Qt) * q.rb * (size_t)(q.seg ? 1 : q.R);
    // resident workgroups per CU: LDS copies of the LUT, and the register allocation's waves per SIMD
    const int per_cu = std::max(1, std::min<int>((int)(c->lds_bytes / lds), (K2V3_WAVES * 4 * 64) / K2V3_THREADS));
    const int64_t nblocks = (q.nreads + q.rpb - 1) / q.rpb;
    const int64_t want = (nblocks + (K2V3_THREADS / 64) - 1) / (K2V3_THREADS / 64);
    const int gx = (int)std::min<int64_t>(want, std::max<int64_t>(1, (int64_t)c->cus * per_cu / slices));
    return launch_lds(c, 1, LDS_KERNELS[errbit ? LK_K2V3_NIB_EB : nib ? LK_K2V3_NIB : LK_K2V3], dim3((unsigned)std::max(gx, 1), (unsigned)slices, 1), dim3(K2V3_THREADS), lds, &q);
}

static int apply_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                      int64_t nrows, int pitch, int pairs, int R, int S2, int minscore, const void* d_lut_blob,
                      const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out, int nib = 0, const int64_t* d_perm = nullptr, int errbit = 0);

int kbbq_apply_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                   int64_t nreads, int pitch, int R, int Qt, int S2, int minscore,
                   const void* d_lut, int mode, uint8_t* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_apply_dev", nreads, pitch, d_seq, d_qual, d_out);
    if (rc) return rc;
    if (R <= 0 || R > 32767 || Qt <= 0 || Qt > 95 || S2 <= 0 || S2 > 65536)
        return fail(KBBQ_E_ARG, "kbbq_apply_dev: bad table shape R=%d Qt=%d S2=%d (Qt <= 95)", R, Qt, S2);
    if (minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "kbbq_apply_dev: minscore out of range");
    if ((uintptr_t)d_lut & 15) return fail(KBBQ_E_ARG, "kbbq_apply_dev: LUT must be 16-byte aligned");
    if (mode != KBBQ_APPLY_CHECKED && mode != KBBQ_APPLY_FAST) return fail(KBBQ_E_ARG, "kbbq_apply_dev: bad mode %d", mode);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    const int64_t nblocks = (nreads + 63) / 64;

    // the LUT of the columns rows of this pitch can reach (narrowed_row_lut): a band of short reads under wide tables
    const int Sb = row_lut_width(pitch, S2);
    const size_t full_bytes = (size_t)R * (33 + Qt) * full_lut_row_bytes(Sb);
    // one read group, rows as a caller holds them (one character row per read): the short-lived kernel through apply_rows when it
    // serves them.  What it cannot serve (a foreign letter, q > 42, a read longer than the LUT, a read group other than 0 -- and,
    // because it screens whole 16-byte chunks, a byte other than 'N' in the sequence padding of a read's last chunk) it reports as
    // KBBQ_E_LUT with no read index: a KBBQ_APPLY_CHECKED run over the same rows decides, as for a LUT that is not range-safe.
    // Who re-runs: the caller of this entry point (kbbq/_device.py apply); kbbq_apply does it itself (stage_run's `exact`).
    if (mode == KBBQ_APPLY_FAST && R == 1 && Qt == KQ && !(S2 & 1) && S2 <= 65534
        && k2_tile_serves(c, 0, 0, R, false, pitch / 16, (size_t)(33 + KQ) * full_lut_row_bytes(Sb)))
        return apply_rows(c, "kbbq_apply_dev", d_seq, d_qual, d_meta, nreads, pitch, 0, R, S2, minscore, d_lut, nullptr, nullptr, d_out, 0, nullptr);
    if (mode == KBBQ_APPLY_FAST && full_bytes <= (size_t)c->lds_bytes) {
        // the persistent kernel as apply_rows launches it, for any Qt and an odd S2 too (apply_rows takes neither)
        K2v3Params q = k2v3_params(c, d_seq, d_qual, d_meta, nreads, pitch, 0, R, Qt, S2, Sb, minscore, d_lut, nullptr, nullptr, nullptr, d_out);
        if (!narrowed_row_lut(c, d_lut, R, Qt, S2, Sb, minscore, &q.full)) return fail(KBBQ_E_HIP, "kbbq_apply_dev: no scratch for the narrowed LUT");
        return launch_k2v3(c, q, 0);
    }

    K2Params p;
    p.seq = d_seq; p.qual = d_qual; p.meta = d_meta; p.nreads = nreads; p.pitch = pitch;
    p.cpr = pitch / 16; p.cpr_magic = magic_for(p.cpr);
    p.R = R; p.Qt = Qt; p.S2 = S2; p.minscore = minscore; p.qlo = 33u + (u32)minscore;
    p.lut = reinterpret_cast<const int16_t*>(d_lut); p.lut_count = (int)kbbq_lut_count(R, Qt, S2);
    p.out = d_out; p.status = c->d_status;
    // FAST (flags == 0): every value fits int8 -> stage the one-byte copy; CHECKED: the int16 LUT.
    // Too big for LDS either way: per-base exact path from global memory.
    const bool fast = mode == KBBQ_APPLY_FAST;
    const size_t stage_bytes = fast ? lut_compact8_bytes(R, Qt, S2) : (size_t)p.lut_count * 2;
    const bool in_lds = stage_bytes + 16 <= (size_t)c->lds_bytes;
    p.lut_in_lds = in_lds ? 1 : 0;
    p.stage = fast ? (const void*)(reinterpret_cast<const char*>(d_lut) + lut_compact8_offset(R, Qt, S2)) : d_lut;
    p.stage_bytes = (int)stage_bytes;
    const size_t lds = in_lds ? ((stage_bytes + 15) & ~(size_t)15) : 0;
    // 256-thread workgroups while >= 4 of them fit a CU, else 1024-thread ones (same waves per CU)
    int threads = 256, per_cu = 8;
    if (in_lds) {
        per_cu = (int)(c->lds_bytes / lds);
        if (per_cu < 4) { threads = 1024; per_cu = std::min(per_cu, 2); }
        per_cu = std::max(1, std::min(per_cu, 2048 / threads));
    }
    const int64_t want = (nblocks + (threads / 64) - 1) / (threads / 64);
    int gx = (int)std::min<int64_t>(want, (int64_t)c->cus * per_cu);
    dim3 grid((unsigned)std::max(gx, 1), 1, 1), block((unsigned)threads, 1, 1);
    if (in_lds) return launch_lds(c, 1, LDS_KERNELS[fast ? LK_K2_LDS8 : LK_K2_LDS16], grid, block, lds, &p);
    {
        Timed t(c, 1);
        hipLaunchKernelGGL((k2_apply<int16_t, false, true>), grid, block, 0, c->stream, p);       // the LUT stays in global memory: no LDS
    }
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_synth_dev(kbbq_ctx* c, uint8_t* d_seq, uint8_t* d_cseq, uint8_t* d_qual, uint32_t* d_meta,
                   int64_t first, int64_t nreads, int64_t total, int pitch, uint64_t seed,
                   int len_lo, int len_hi, int nrg, int qlo, int qhi, const uint32_t* thr43)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_synth_dev", nreads, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (len_lo < 0 || len_hi < len_lo || len_hi > pitch || nrg <= 0 || nrg > 32767 || qlo < 0 || qhi < qlo || qhi >= KQ || total <= 0)
        return fail(KBBQ_E_ARG, "kbbq_synth_dev: bad shape");
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    KSParams p;
    p.seq = d_seq; p.cseq = d_cseq; p.qual = d_qual; p.meta = d_meta;
    p.first = first; p.nreads = nreads; p.total = total; p.pitch = pitch; p.cpr = pitch / 16;
    p.seed = seed; p.len_lo = len_lo; p.len_hi = len_hi; p.nrg = nrg; p.qlo = qlo; p.qhi = qhi;
    memcpy(p.thr, thr43, sizeof p.thr);
    const int64_t nchunks = nreads * p.cpr;
    int gx = (int)std::min<int64_t>((nchunks + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(ks_synth, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// ---- K3: model solve ------------------------------------------------------
static int load_consts(SolveConsts& c, const double* h_consts)
{
    if (!h_consts) return fail(KBBQ_E_ARG, "model constants are NULL");
    memcpy(c.prior, h_consts, sizeof c.prior);
    memcpy(c.logp, h_consts + KSOLVE_NQ, sizeof c.logp);
    memcpy(c.log1mp, h_consts + 2 * KSOLVE_NQ, sizeof c.log1mp);
    return KBBQ_OK;
}

int kbbq_delta_q_dev(kbbq_ctx* c, const int64_t* d_prior_q, const int64_t* d_errs, const int64_t* d_total,
                     const double* d_comb, int64_t ncells, const double* h_consts129, int64_t* d_dq)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (ncells < 0) return fail(KBBQ_E_ARG, "kbbq_delta_q_dev: ncells < 0");
    if (ncells == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K3CellParams p;
    p.prior_q = (const long long*)d_prior_q; p.errs = (const long long*)d_errs; p.total = (const long long*)d_total;
    p.comb = d_comb; p.n = ncells; p.dq = (long long*)d_dq;
    int rc = load_consts(p.c, h_consts129);
    if (rc) return rc;
    int gx = (int)std::min<int64_t>((ncells + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k3_delta_q, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_posterior_q_dev(kbbq_ctx* c, const double* d_prior_q, const int64_t* d_errs, const int64_t* d_total,
                         const double* d_comb, int64_t ncells, const double* h_consts129, int64_t* d_post)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (ncells < 0) return fail(KBBQ_E_ARG, "kbbq_posterior_q_dev: ncells < 0");
    if (ncells == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K3PostParams p;
    p.prior_q = d_prior_q; p.errs = (const long long*)d_errs; p.total = (const long long*)d_total;
    p.comb = d_comb; p.n = ncells; p.post = (long long*)d_post;
    int rc = load_consts(p.c, h_consts129);
    if (rc) return rc;
    int gx = (int)std::min<int64_t>((ncells + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k3_posterior_q, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

size_t kbbq_solve_aux_count(int R, int S2) { return (size_t)R + (size_t)R * KQ + (size_t)R * KQ * S2 + (size_t)R * KQ * KND; }
size_t kbbq_solve_dq_count(int R, int S2) { return (size_t)R + (size_t)R * KQ + (size_t)R * KQ * S2 + (size_t)R * KQ * 17; }

static int launch_solve(kbbq_ctx* c, K3FusedParams& p, int minscore);

int kbbq_solve_dev(kbbq_ctx* c, const int64_t* d_tables, int R, int S2, int minscore, const int32_t* d_meanq,
                   const double* d_aux, const double* h_consts129, int32_t* d_post_q,
                   void* d_lut, int32_t* d_dq)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (R <= 0 || R > 32767 || S2 <= 0 || S2 > 65536) return fail(KBBQ_E_ARG, "kbbq_solve_dev: bad shape R=%d S2=%d", R, S2);
    if (!d_tables || !d_meanq || !d_aux || !d_post_q || !d_lut) return fail(KBBQ_E_ARG, "kbbq_solve_dev: NULL device pointer");
    HIPCHK(hipSetDevice(c->device));
    K3FusedParams p;
    p.tables = (const long long*)d_tables; p.R = R; p.S2 = S2; p.rs = lut_row_stride(S2);
    p.meanq = d_meanq; p.aux = d_aux; p.post_q = d_post_q; p.lut = reinterpret_cast<int16_t*>(d_lut); p.dq = d_dq;
    p.logtab = nullptr; p.meanq_out = nullptr; p.status = c->d_status;
    memset(p.perr, 0, sizeof p.perr);
    int rc = load_consts(p.c, h_consts129);
    if (rc) return rc;
    return launch_solve(c, p, minscore);
}

static int launch_solve(kbbq_ctx* c, K3FusedParams& p, int minscore)
{
    const int R = p.R, S2 = p.S2;
    void* d_lut = p.lut;
    hipLaunchKernelGGL(k3_levels_ab, dim3((unsigned)R), dim3(1024), 0, c->stream, p);
    const int64_t cells = (int64_t)R * KQ * ((int64_t)S2 + KND);              // one wave per cell
    int gx = (int)std::min<int64_t>((cells + 3) / 4, (int64_t)c->cus * 32);
    hipLaunchKernelGGL(k3_level_c, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    // derive the table-driven (int8) LUT and the flags the fast apply kernel relies on
    LutFillParams f;
    f.lut16 = p.lut; f.rs16 = p.rs; f.R = R; f.Qt = KQ; f.S2 = S2; f.minscore = std::min(std::max(minscore, 0), KQ);
    f.full = reinterpret_cast<int8_t*>(d_lut) + lut_full_offset(R, KQ, S2);
    f.compact8 = reinterpret_cast<int8_t*>(d_lut) + lut_compact8_offset(R, KQ, S2);
    f.flags = reinterpret_cast<int*>(reinterpret_cast<char*>(d_lut) + lut_flags_offset(R, KQ, S2));
    f.status = c->d_status;
    HIPCHK(hipMemsetAsync(f.flags, 0, 16, c->stream));
    hipLaunchKernelGGL(k3_fill_full_lut, dim3((unsigned)(R * (33 + KQ))), dim3(256), 0, c->stream, f);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_solve_device_dev(kbbq_ctx* c, const int64_t* d_tables, int R, int S2, int minscore, const double* d_logtab,
                          const double* h_consts172, int32_t* d_post_q, void* d_lut, int32_t* d_dq, int32_t* d_meanq_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (R <= 0 || R > 32767 || S2 <= 0 || S2 > 65536) return fail(KBBQ_E_ARG, "kbbq_solve_device_dev: bad shape R=%d S2=%d", R, S2);
    if (!d_tables || !d_logtab || !h_consts172 || !d_post_q || !d_lut) return fail(KBBQ_E_ARG, "kbbq_solve_device_dev: NULL pointer");
    HIPCHK(hipSetDevice(c->device));
    K3FusedParams p;
    p.tables = (const long long*)d_tables; p.R = R; p.S2 = S2; p.rs = lut_row_stride(S2);
    p.meanq = nullptr; p.aux = nullptr; p.post_q = d_post_q; p.lut = reinterpret_cast<int16_t*>(d_lut); p.dq = d_dq;
    p.logtab = d_logtab; p.meanq_out = d_meanq_out; p.status = c->d_status;
    memcpy(p.perr, h_consts172 + 3 * KSOLVE_NQ, sizeof p.perr);
    int rc = load_consts(p.c, h_consts172);
    if (rc) return rc;
    return launch_solve(c, p, minscore);
}

int kbbq_gammaln_dev(kbbq_ctx* c, const double* d_x, int64_t n, const double* d_logtab, double* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (n < 0 || (n > 0 && (!d_x || !d_out)) || !d_logtab) return fail(KBBQ_E_ARG, "kbbq_gammaln_dev: bad argument");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K3GammalnParams p; p.x = d_x; p.n = n; p.logtab = d_logtab; p.out = d_out;
    int gx = (int)std::min<int64_t>((n + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k3_gammaln, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// workgroups of a streaming kernel with a grid-stride loop: `per_cu` per CU.  Measured in three interleaved rounds (scripts/gpu_grids.sh,
// DESIGN.md section 6): 64 per CU -- four generations of workgroups per CU slot -- beat the 8-16 these kernels
// started with by 6-13 % (K4 1.95 -> 1.83 ms, K5 1.12 -> 0.98, K6 2.66 -> 2.37 per 16 M reads), 256 did for the layout pass
// (9.46 -> 8.42 ms per 50 M reads); one item per thread loses again where a workgroup has set-up work (K4's queue, K5's
// LDS counters and their flush: 13 ms).
static int bounded_grid(int64_t want, const kbbq_ctx* c, int per_cu)
{
    const int64_t cap = (int64_t)c->cus * per_cu;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, cap));
}

// ---- mate-pair rows ---------------------------------------------------------
int kbbq_pair_pitch(int S2) { return pair_pitch(S2); }
size_t kbbq_pair_lut_bytes(int R, int Qt, int S2) { return (size_t)R * (33 + Qt) * pair_lut_row_bytes(S2); }

static int check_pairs(const char* who, int64_t npairs, int S2)
{
    if (npairs < 0) return fail(KBBQ_E_ARG, "%s: npairs < 0", who);
    if (S2 <= 0 || (S2 & 1) || S2 > 65534) return fail(KBBQ_E_ARG, "%s: S2 must be positive and even (%d)", who, S2);
    return KBBQ_OK;
}

int kbbq_pack_pairs_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                        const uint32_t* d_meta, int64_t npairs, int pitch, int S2,
                        uint8_t* d_pseq, uint8_t* d_pcseq, uint8_t* d_pqual, uint32_t* d_pmeta)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_pack_pairs_dev", npairs, S2);
    if (rc) return rc;
    if (pitch <= 0 || (pitch & 15) || pitch < S2 / 2) return fail(KBBQ_E_ARG, "kbbq_pack_pairs_dev: bad pitch %d", pitch);
    if (!d_seq || !d_qual || !d_meta || !d_pseq || !d_pqual || !d_pmeta || (d_cseq && !d_pcseq))
        return fail(KBBQ_E_ARG, "kbbq_pack_pairs_dev: NULL pointer");
    if (((uintptr_t)d_pseq | (uintptr_t)d_pcseq | (uintptr_t)d_pqual) & 15) return fail(KBBQ_E_ARG, "kbbq_pack_pairs_dev: planes must be 16-byte aligned");
    if (npairs == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    PairPackParams p;
    p.src[0] = d_seq; p.src[1] = d_cseq; p.src[2] = d_qual;
    p.dst[0] = d_pseq; p.dst[1] = d_pcseq; p.dst[2] = d_pqual;
    p.fill[0] = 'N'; p.fill[1] = 'N'; p.fill[2] = 0;
    p.meta = d_meta; p.pmeta = d_pmeta; p.npairs = npairs; p.pitch = pitch; p.ppitch = pair_pitch(S2); p.S = S2 / 2; p.unpack = 0;
    const int64_t nchunks = npairs * (p.ppitch / 16);
    const int gx = bounded_grid((nchunks + 255) / 256, c, 256);
    hipLaunchKernelGGL(k7_pack_pairs, dim3((unsigned)gx), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_unpack_pairs_dev(kbbq_ctx* c, const uint8_t* d_pplane, int64_t npairs, int S2, int pitch, uint8_t* d_plane)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_unpack_pairs_dev", npairs, S2);
    if (rc) return rc;
    if (pitch <= 0 || (pitch & 15) || pitch < S2 / 2) return fail(KBBQ_E_ARG, "kbbq_unpack_pairs_dev: bad pitch %d", pitch);
    if (!d_pplane || !d_plane || ((uintptr_t)d_plane & 15)) return fail(KBBQ_E_ARG, "kbbq_unpack_pairs_dev: bad pointer");
    if (npairs == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    PairPackParams p;
    p.src[0] = d_pplane; p.src[1] = nullptr; p.src[2] = nullptr; p.dst[0] = d_plane; p.dst[1] = nullptr; p.dst[2] = nullptr;
    p.fill[0] = p.fill[1] = p.fill[2] = 0;
    p.meta = nullptr; p.pmeta = nullptr; p.npairs = npairs; p.pitch = pitch; p.ppitch = pair_pitch(S2); p.S = S2 / 2; p.unpack = 1;
    const int64_t nchunks = 2 * npairs * (pitch / 16);
    const int gx = bounded_grid((nchunks + 255) / 256, c, 256);
    hipLaunchKernelGGL(k7_pack_pairs, dim3((unsigned)gx), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// K1's LDS beside `dn` copies of the context table, once the cycle rows are laid out (q.row_bytes, q.slack_bytes): several
// trash rows first (K1v3Params::ntrash: the padding behind every read's last base is the hotter spot), then copies of the cycle
// table for rows of up to 12 chunks (K1v3Params::pos_copies: wider rows spread a wave's lanes over enough columns), as many of
// 8 / 4 / 2 and 4 / 2 as the LDS holds; KBBQ_K1_NTRASH / KBBQ_K1_POSCOPIES cap them (=1: none).  Returns the LDS bytes.
static size_t k1_lds_plan(K1v3Params& q, int dn, const kbbq_ctx* c)
{
    auto bytes_for = [&](int nt, int pc) {
        const size_t rows = (size_t)q.nrows - 1 + nt;
        return rows * 128 * dn + (size_t)pc * (rows * q.row_bytes + q.slack_bytes);
    };
    const char* nt_env = getenv("KBBQ_K1_NTRASH");
    const char* pc_env = getenv("KBBQ_K1_POSCOPIES");
    const int most_t = nt_env ? atoi(nt_env) : 8, most = pc_env ? atoi(pc_env) : 4;
    q.ntrash = 1; q.pos_copies = 1;
    for (int nt = 8; nt >= 2; nt >>= 1)
        if (nt <= most_t && bytes_for(nt, 1) <= (size_t)c->lds_bytes) { q.ntrash = nt; break; }
    if (q.cpr <= 12)
        for (int pc = 4; pc >= 2; pc >>= 1)
            if (pc <= most && bytes_for(q.ntrash, pc) <= (size_t)c->lds_bytes) { q.pos_copies = pc; break; }
    q.pos_copy_bytes = (u32)((size_t)(q.nrows - 1 + q.ntrash) * q.row_bytes + q.slack_bytes);
    return bytes_for(q.ntrash, q.pos_copies);
}

// One attempt at K1's LDS geometry: `copies` of the context table beside cycle rows of 3S - cut words (3S words serve reads
// of any length: one word per first-in-pair position [0, S) and per second-in-pair index S + 2(S - len) + pos <= 3S - len - 1).
// False: the tables do not fit the LDS, or the 16-bit packed context counts could overflow between two flushes.
static bool k1_geometry(K1v3Params& q, const kbbq_ctx* c, int copies, int cut, int minlen)
{
    q.row_bytes = (u32)((3 * q.S - cut) | 1) * 4u;
    q.minlen = minlen;
    // bytes past a read's end (quality 0) land on the trash row, the last one, at indexes up to 3S - cut - 1 + 15
    q.slack_bytes = (u32)(q.S + 32) * 4u;
    q.dn_flush_iters = std::max(1, 65535 / ((K1V3_THREADS / copies) * 16 * q.cpr));
    const size_t lds = (size_t)q.nrows * 128 * copies + (size_t)q.nrows * q.row_bytes + q.slack_bytes;
    return lds <= (size_t)c->lds_bytes && (K1V3_THREADS / copies) * 16 * q.cpr <= 65535;
}

static bool k1_split(const K1v3Params& q) { return q.type_minscore > q.minscore; }
// iterations one workgroup per read group would make over the rows: no launch has more workgroups per group than this
static int64_t k1_iters(const K1v3Params& q) { return ((q.nreads + 63) / 64 + (K1V3_THREADS / 64) - 1) / (K1V3_THREADS / 64); }

// K1 on the rows of su.q: one 16-wave workgroup per CU, the read groups side by side in grid.y
static int launch_k1(kbbq_ctx* c, K1Form form, const K1Setup& su, int nib)
{
    const int gx = (int)std::min<int64_t>(k1_iters(su.q), std::max(1, c->cus / su.q.R));
    return launch_lds(c, 0, k1_kernel(form, k1_split(su.q), su.dn, nib, su.kj, su.eb), dim3((unsigned)gx, (unsigned)su.q.R, 1), dim3(K1V3_THREADS),
                      su.lds, &su.q);
}

// K1 (table-driven kernel) on one-read-per-row or mate-pair rows, optionally grouped by read group
static int accumulate_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                           const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2, int minscore,
                           int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables, bool* fits, int S_band, int S_min, int nib, int twins,
                           K1Setup* setup_only, int errbit)
{
    if (fits) *fits = true;
    if (S_band < 0 || S_band > S2 / 2 || (pairs && S_band)) return fail(KBBQ_E_ARG, "%s: S_band out of range (%d)", who, S_band);
    if (S_min < 0 || S_min > (S_band ? S_band : S2 / 2)) return fail(KBBQ_E_ARG, "%s: S_min out of range (%d)", who, S_min);
    // KBBQ_ROWS_ERRBIT: the corrected plane is not read (and may be NULL); only the joint-row forms below know the flag
    if (errbit) d_cseq = nullptr;
    if (errbit && !(pairs && nib && (pitch == 16 * 19 || pitch == 16 * 13)))
        return fail(KBBQ_E_ARG, "%s: KBBQ_ROWS_ERRBIT describes 4-bit mate-pair rows of 19 or 13 chunks (pitch %d)", who, pitch);
    int rc = check_planes(who, nrows, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (R <= 0 || R > 32767) return fail(KBBQ_E_ARG, "%s: R out of range (%d)", who, R);
    if (S2 <= 0 || (S2 & 1) || S2 > 65534) return fail(KBBQ_E_ARG, "%s: S2 must be positive and even (%d)", who, S2);
    if (minscore < 0 || minscore > KQ - 1) return fail(KBBQ_E_ARG, "%s: minscore out of range (%d)", who, minscore);
    if (dinuc_minscore < 0 || dinuc_minscore > 222) return fail(KBBQ_E_ARG, "%s: dinuc_minscore out of range (%d)", who, dinuc_minscore);
    if (pairs && pitch != pair_pitch(S2)) return fail(KBBQ_E_ARG, "%s: mate-pair rows of %d-base reads have pitch %d, not %d", who, S2 / 2, pair_pitch(S2), pitch);
    if (nrows == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    const int S = S_band ? S_band : S2 / 2;          // the LDS tables are laid out for the longest read of THIS batch
    K1Setup su;
    K1v3Params& q = su.q;
    q.aflags = nullptr; q.aclip = nullptr; q.atrim = nullptr;
    q.seq = d_seq; q.cseq = d_cseq; q.qual = d_qual; q.meta = d_meta;
    q.nreads = nrows; q.pitch = pitch; q.cpr = pitch / 16; q.cpr_magic = magic_for(q.cpr);
    q.R = R; q.S = S; q.gS2 = S2; q.minscore = minscore; q.type_minscore = dinuc_minscore;
    q.qlo_m1 = 32u + (u32)minscore; q.dlo = 33u + (u32)dinuc_minscore;
    q.nrows = KQ + 1 - minscore;
    q.maxlen = pairs ? S2 + 1 : S; q.gap = pairs ? 1 : 0; q.twins = (pairs && twins) ? 1 : 0;
    q.seg = reinterpret_cast<const long long*>(d_seg);
    q.tables = reinterpret_cast<u64*>(d_tables); q.status = c->d_status;
    q.genome = nullptr; q.ag0 = nullptr;
    // LDS geometry (k1_geometry).  When 3S words per cycle row do not fit (reads of ~200 bases and more), a band whose shortest
    // read is S_min needs only 3S - S_min words, and 8 copies of the context table instead of 16 free the rest: reads of up to
    // ~300 bases still run this kernel.
    const int trim = (!pairs && S_min > 0) ? std::min(S_min, S) : 0;
    // mate-pair rows of 19 or 13 chunks (2 x 150, 2 x 100 bp) on 4-bit planes: the chunk-position-major cycle table (kernel comment), the
    // 13-chunk form with 8 trash rows (K1v3Params::ntrash; 19 chunks were measured with 4 and 8 of them: nothing).  Measured for the other
    // lengths instruments emit (profiles/): 2 x 100 bp 1.37 -> 1.31 ms per 3 Gbases; 2 x 50 bp (7 chunks) is FASTER position-major with its
    // copies of the cycle table (1.52 against 1.64 ms); 2 x 75 / 2 x 125 / 2 x 250 bp never take mate-pair rows (2 S + 1 rounds up to
    // twice the single read's pitch: no bytes saved).
    if (pairs && nib && (q.cpr == 19 || q.cpr == 13)) {
        // joint rows (k1v3_body): a quality's cycle words, then its 32 context slots x 16 copies -- 832 / 736 words, multiples of 32
        q.row_bytes = (u32)((((16 * q.cpr + 31) & ~31) + 32 * K1V3_DNREP) * 4);
        q.minlen = 0; q.slack_bytes = 0; q.pos_copies = 1;
        q.dn_flush_iters = std::max(1, 65535 / ((K1V3_THREADS / K1V3_DNREP) * 16 * q.cpr));
        for (int nt = q.cpr == 19 ? 1 : 8; nt >= 1 && !su.dn; nt >>= 1) {
            const size_t rows = (size_t)q.nrows - 1 + nt;
            su.lds = rows * q.row_bytes;
            if (su.lds > (size_t)c->lds_bytes) continue;
            su.dn = K1V3_DNREP; su.kj = q.cpr; su.eb = errbit ? 1 : 0;       // the form applies AND its tables fit
            q.ntrash = nt; q.pos_copy_bytes = (u32)(rows * q.row_bytes);
        }
    }
    // (44 rows of 3328 / 2944 bytes at most: they fit the 160 KB of a gfx950 CU.  A guard, not a fallback: no other form of K1 knows the flag)
    if (errbit && !su.kj) return fail(KBBQ_E_ARG, "%s: the joint-row tables of KBBQ_ROWS_ERRBIT rows do not fit the LDS (%d bytes)", who, c->lds_bytes);
    for (int attempt = 0; attempt < (trim ? 3 : 1) && !su.dn; ++attempt) {
        const int copies = attempt == 2 ? 8 : K1V3_DNREP, cut = attempt ? trim : 0;
        if (k1_geometry(q, c, copies, cut, cut)) su.dn = copies;
    }
    if (!su.dn) {
        if (fits) { *fits = false; return KBBQ_OK; }     // the caller has another kernel for this shape
        return fail(KBBQ_E_LUT, "%s: %d-base reads with minscore %d do not fit the LDS tables; use plain one-read-per-row planes", who, S, minscore);
    }
    if (!su.kj) su.lds = k1_lds_plan(q, su.dn, c);
    if (setup_only) { *setup_only = su; return KBBQ_OK; }
    return launch_k1(c, K1_ROWS, su, nib);
}

int kbbq_accumulate_pairs_dev(kbbq_ctx* c, const uint8_t* d_pseq, const uint8_t* d_pcseq, const uint8_t* d_pqual,
                              const uint32_t* d_pmeta, int64_t npairs, int R, int S2, int minscore,
                              int dinuc_minscore, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_accumulate_pairs_dev", npairs, S2);
    if (rc) return rc;
    return accumulate_rows(c, "kbbq_accumulate_pairs_dev", d_pseq, d_pcseq, d_pqual, d_pmeta, npairs, pair_pitch(S2), 1,
                           R, S2, minscore, dinuc_minscore, nullptr, d_tables, nullptr);
}

int kbbq_accumulate_grouped_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                                const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2, int S_band,
                                int S_min, int minscore, int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_seg) return fail(KBBQ_E_ARG, "kbbq_accumulate_grouped_dev: d_seg is NULL");
    return accumulate_rows(c, "kbbq_accumulate_grouped_dev", d_seq, d_cseq, d_qual, d_meta, nrows, pitch, pairs ? 1 : 0,
                           R, S2, minscore, dinuc_minscore, d_seg, d_tables, nullptr, S_band, S_min);
}

int kbbq_pair_lut_dev(kbbq_ctx* c, const void* d_lut_blob, int R, int S2, int minscore, void* d_pair_lut)
{
    return kbbq_pair_lut_rows_dev(c, d_lut_blob, R, S2, minscore, KBBQ_ROWS_PAIRS, d_pair_lut);
}

int kbbq_pair_lut_rows_dev(kbbq_ctx* c, const void* d_lut_blob, int R, int S2, int minscore, int flags, void* d_pair_lut)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_pair_lut_dev", 0, S2);
    if (rc) return rc;
    if (!(flags & KBBQ_ROWS_PAIRS) || (flags & ~(KBBQ_ROWS_PAIRS | KBBQ_ROWS_NIBBLES | KBBQ_ROWS_TWINS | KBBQ_ROWS_ERRBIT)))
        return fail(KBBQ_E_ARG, "kbbq_pair_lut_rows_dev: flags 0x%x are not those of mate-pair rows", flags);
    if (R <= 0 || R > 32767 || !d_lut_blob || !d_pair_lut) return fail(KBBQ_E_ARG, "kbbq_pair_lut_dev: bad argument");
    HIPCHK(hipSetDevice(c->device));
    PairLutParams f;
    f.lut16 = reinterpret_cast<const int16_t*>(d_lut_blob); f.rs16 = lut_row_stride(S2); f.R = R; f.Qt = KQ; f.S2 = S2;
    f.minscore = std::min(std::max(minscore, 0), KQ);
    f.twins = (flags & KBBQ_ROWS_TWINS) ? 1 : 0;
    f.out = reinterpret_cast<int8_t*>(d_pair_lut);
    hipLaunchKernelGGL(k3_fill_pair_lut, dim3((unsigned)(R * (33 + KQ))), dim3(256), 0, c->stream, f);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// the short-lived kernel's parameters for the rows and the LUT of `q` (no workgroup plan: one read group, all rows)
static K2tParams k2t_params(const K2v3Params& q)
{
    K2tParams t;
    t.seq = q.seq; t.qual = q.qual; t.meta = q.meta; t.nchunks = q.nreads * q.cpr; t.cpr = q.cpr; t.cpr_magic = q.cpr_magic;
    t.Qt = q.Qt; t.S2 = q.S2; t.maxlen = q.maxlen; t.lut = q.full; t.lut_bytes = (int)(((size_t)(33 + q.Qt) * q.rb + 15) & ~(size_t)15);
    t.rb = q.rb; t.ctx_off = q.ctx_off; t.W = q.W; t.seg = q.seg; t.R = q.R; t.wg_start = nullptr; t.order = nullptr;
    t.perm = q.perm; t.pitch = q.pitch; t.out = q.out; t.status = q.status;
    t.xcd_tiles = K2T_XCD_TILES;
    return t;
}

// K2 (table-driven kernel) on one-read-per-row or mate-pair rows, optionally grouped by read group
static int apply_rows(kbbq_ctx* c, const char* who, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                      int64_t nrows, int pitch, int pairs, int R, int S2, int minscore, const void* d_lut_blob,
                      const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out, int nib, const int64_t* d_perm, int errbit)
{
    int rc = check_planes(who, nrows, pitch, d_seq, d_qual, d_out);
    if (rc) return rc;
    if (errbit && !(pairs && nib && (pitch == 16 * 19 || pitch == 16 * 13)))
        return fail(KBBQ_E_ARG, "%s: KBBQ_ROWS_ERRBIT describes 4-bit mate-pair rows of 19 or 13 chunks (pitch %d)", who, pitch);
    if (R <= 0 || R > 32767 || !d_lut_blob || (pairs && (!d_pair_lut || ((uintptr_t)d_pair_lut & 15)))) return fail(KBBQ_E_ARG, "%s: bad argument", who);
    if (S2 <= 0 || (S2 & 1) || S2 > 65534) return fail(KBBQ_E_ARG, "%s: S2 must be positive and even (%d)", who, S2);
    if (minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "%s: minscore out of range", who);
    if (pairs && pitch != pair_pitch(S2)) return fail(KBBQ_E_ARG, "%s: mate-pair rows of %d-base reads have pitch %d, not %d", who, S2 / 2, pair_pitch(S2), pitch);
    // one read per row: the LUT of the columns rows of this pitch can reach (narrowed_row_lut)
    const int Sb = pairs ? S2 : row_lut_width(pitch, S2);
    K2v3Params q = k2v3_params(c, d_seq, d_qual, d_meta, nrows, pitch, pairs, R, KQ, S2, Sb, minscore, d_lut_blob, d_pair_lut, d_seg, d_perm, d_out);
    const size_t rg_bytes = (size_t)(33 + KQ) * q.rb;
    const size_t lds = d_seg ? rg_bytes : rg_bytes * (size_t)R;
    if (lds > (size_t)c->lds_bytes)
        return fail(KBBQ_E_LUT, "%s: the apply LUT (%zu B) does not fit the LDS; group the rows by read group or use kbbq_apply_dev", who, lds);
    if (nrows == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    if (!pairs && !narrowed_row_lut(c, d_lut_blob, R, KQ, S2, Sb, minscore, &q.full)) return fail(KBBQ_E_HIP, "%s: no scratch for the narrowed LUT", who);
    if (!k2_tile_serves(c, pairs, nib, R, d_seg != nullptr, q.cpr, rg_bytes)) return launch_k2v3(c, q, nib, errbit);

    K2tParams t = k2t_params(q);
    const int64_t per_wg = (int64_t)(K2T_THREADS / 64) * 64 * K2T_STEPS;
    int64_t gt = (t.nchunks + per_wg - 1) / per_wg;
    if (d_seg) {
        gt += R;                                     // every group rounds its last workgroup up
        const bool interleave = d_perm && R > 1;
        const int64_t ints = (int64_t)(R + 1) + 1 + (interleave ? 2 * gt : 0);
        if (ints > 0x7FFFFFFF) return fail(KBBQ_E_ARG, "%s: too many workgroups", who);
        rc = grow_scratch(c, c->wgplan, (size_t)ints * sizeof(int));
        if (rc) return rc;
        int* wg_start = reinterpret_cast<int*>(c->wgplan.p);
        K2tPlanParams pl; pl.seg = t.seg; pl.R = R; pl.cpr = q.cpr; pl.wg_start = wg_start;
        hipLaunchKernelGGL(k2t_plan, dim3(1), dim3(64), 0, c->stream, pl);
        t.wg_start = wg_start;
        if (interleave) {
            K2tOrderParams op; op.wg_start = wg_start; op.R = R;
            op.xcd = K2T_XCD;
            op.order = reinterpret_cast<int2*>(wg_start + ((R + 2) & ~1));           // 8-byte aligned behind the starts
            hipLaunchKernelGGL(k2t_order, dim3((unsigned)((gt + 255) / 256)), dim3(256), 0, c->stream, op);
            t.order = op.order;
        }
    }
    // 4-bit mate-pair rows of 19 / 13 chunks: the instance with that geometry compiled in (K1's KJ instances' counterpart)
    const int kj = (pairs && nib) ? k2t_pair_form(t) : 0;
    if (kj < 0) return fail(KBBQ_E_ARG, "%s: mate-pair rows of %d chunks do not have the geometry k2t_apply_pair was compiled for", who, q.cpr);
    if (errbit && kj <= 0) return fail(KBBQ_E_ARG, "%s: no instance of K2 reads KBBQ_ROWS_ERRBIT rows of %d chunks", who, q.cpr);
    const LdsKernel k = kj == 19 ? (errbit ? LK_K2T_PAIR19_EB : LK_K2T_PAIR19) : kj == 13 ? (errbit ? LK_K2T_PAIR13_EB : LK_K2T_PAIR13)
                        : nib ? LK_K2T_NIB : LK_K2T;
    return launch_lds(c, 1, LDS_KERNELS[k], dim3((unsigned)gt), dim3(K2T_THREADS), (size_t)t.lut_bytes, &t);
}

int kbbq_apply_pairs_dev(kbbq_ctx* c, const uint8_t* d_pseq, const uint8_t* d_pqual, const uint32_t* d_pmeta,
                         int64_t npairs, int R, int S2, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                         uint8_t* d_pout)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_pairs("kbbq_apply_pairs_dev", npairs, S2);
    if (rc) return rc;
    return apply_rows(c, "kbbq_apply_pairs_dev", d_pseq, d_pqual, d_pmeta, npairs, pair_pitch(S2), 1, R, S2, minscore,
                      d_lut_blob, d_pair_lut, nullptr, d_pout);
}

int kbbq_apply_grouped_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                           int64_t nrows, int pitch, int pairs, int R, int S2, int minscore, const void* d_lut_blob,
                           const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_seg) return fail(KBBQ_E_ARG, "kbbq_apply_grouped_dev: d_seg is NULL");
    return apply_rows(c, "kbbq_apply_grouped_dev", d_seq, d_qual, d_meta, nrows, pitch, pairs ? 1 : 0, R, S2, minscore,
                      d_lut_blob, d_pair_lut, d_seg, d_out);
}


// ---- layouts: rows as handed over -> what K1 / K2 run fastest on ------------
// errbit_ok: the call reads (or writes) KBBQ_ROWS_ERRBIT planes -- K1 / K2 on rows, the layout pass, the pair LUT; everything else that
// takes a 4-bit seq plane would read bit 3 as part of a code and refuses the flag
static int layout_flags_ok(const char* who, int flags, bool errbit_ok = false)
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

int kbbq_accumulate_rows_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                             const uint32_t* d_meta, int64_t nrows, int pitch, int flags, int R, int S2, int S_band,
                             int S_min, int minscore, int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = layout_flags_ok("kbbq_accumulate_rows_dev", flags, true);
    if (rc) return rc;
    const int pairs = (flags & KBBQ_ROWS_PAIRS) ? 1 : 0;
    if (pairs) { rc = check_pairs("kbbq_accumulate_rows_dev", nrows, S2); if (rc) return rc; }
    return accumulate_rows(c, "kbbq_accumulate_rows_dev", d_seq, d_cseq, d_qual, d_meta, nrows, pitch, pairs, R, S2, minscore,
                           dinuc_minscore, d_seg, d_tables, nullptr, pairs ? 0 : S_band, pairs ? 0 : S_min,
                           (flags & KBBQ_ROWS_NIBBLES) ? 1 : 0, (flags & KBBQ_ROWS_TWINS) ? 1 : 0, nullptr, (flags & KBBQ_ROWS_ERRBIT) ? 1 : 0);
}

int kbbq_apply_rows_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows,
                        int pitch, int flags, int R, int S2, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                        const int64_t* d_seg, const int64_t* d_perm, uint8_t* d_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = layout_flags_ok("kbbq_apply_rows_dev", flags, true);
    if (rc) return rc;
    const int pairs = (flags & KBBQ_ROWS_PAIRS) ? 1 : 0;
    if (pairs) { rc = check_pairs("kbbq_apply_rows_dev", nrows, S2); if (rc) return rc; }
    return apply_rows(c, "kbbq_apply_rows_dev", d_seq, d_qual, d_meta, nrows, pitch, pairs, R, S2, minscore, d_lut_blob,
                      d_pair_lut, d_seg, d_out, (flags & KBBQ_ROWS_NIBBLES) ? 1 : 0, d_perm, (flags & KBBQ_ROWS_ERRBIT) ? 1 : 0);
}

// ---- all length bands of a mixed-length input in ONE launch per kernel -------------------------------------------
static int band_accumulate_alone(kbbq_ctx* c, const kbbq_band& b, int R, int S2, int minscore, int dinuc_minscore, int64_t* d_tables)
{
    if (b.flags || b.d_seg)
        return kbbq_accumulate_rows_dev(c, b.d_seq, b.d_cseq, b.d_qual, b.d_meta, b.nrows, b.pitch, b.flags, R, S2, b.S_band, b.S_min,
                                        minscore, dinuc_minscore, b.d_seg, d_tables);
    return kbbq_accumulate_band_dev(c, b.d_seq, b.d_cseq, b.d_qual, b.d_meta, b.nrows, b.pitch, R, S2, b.S_band, b.S_min, minscore,
                                    dinuc_minscore, d_tables);
}

// workgroups for every band of a merged launch: one each, the rest of `total` by largest remainder of weight / sum(weight),
// never more than a band can use (`cap`)
static void share_workgroups(const std::vector<double>& weight, const std::vector<int64_t>& cap, int total, std::vector<int>& out)
{
    const size_t n = weight.size();
    out.assign(n, 1);
    int left = total - (int)n;
    double sum = 0; for (double w : weight) sum += w;
    for (int round = 0; round < 4 && left > 0 && sum > 0; ++round) {            // a capped band's surplus goes round again
        std::vector<std::pair<double, size_t>> frac;
        int given = 0; double open_sum = 0;
        for (size_t i = 0; i < n; ++i) if (out[i] < cap[i]) open_sum += weight[i];
        if (open_sum <= 0) break;
        const int pool = left;
        for (size_t i = 0; i < n; ++i) {
            if (out[i] >= cap[i]) continue;
            const double want = pool * weight[i] / open_sum;
            int add = (int)std::min<int64_t>((int64_t)want, cap[i] - out[i]);
            out[i] += add; given += add;
            if (out[i] < cap[i]) frac.push_back({want - (int64_t)want, i});
        }
        left -= given;
        std::sort(frac.begin(), frac.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        for (auto& f : frac) { if (left <= 0) break; if (out[f.second] < cap[f.second]) { ++out[f.second]; --left; } }
    }
}

int kbbq_accumulate_bands_dev(kbbq_ctx* c, const kbbq_band* bands, int nbands, int R, int S2, int minscore, int dinuc_minscore,
                              int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbands < 0 || (nbands > 0 && !bands)) return fail(KBBQ_E_ARG, "kbbq_accumulate_bands_dev: bad band list");
    // which bands the merged kernel (k1v3_bands) takes: the table-driven K1 fits their LDS geometry, position-major cycle
    // table (not the chunk-position-major form of 2 x 150 bp mate-pair rows), all on 4-bit planes or all on character planes
    std::vector<K1Setup> setups; std::vector<int> merged, alone;
    const bool merge = !env_is("KBBQ_K1_BANDS", "0");                // "0": a launch per band (A/B timing)
    int nib_of_merge = -1;
    for (int i = 0; i < nbands; ++i) {
        const kbbq_band& b = bands[i];
        if (b.nrows == 0) continue;
        int rc = layout_flags_ok("kbbq_accumulate_bands_dev", b.flags, true);      // (an ERRBIT band is a KJ form: it goes alone, never into k1v3_bands)
        if (rc) return rc;
        const int pairs = (b.flags & KBBQ_ROWS_PAIRS) ? 1 : 0, nib = (b.flags & KBBQ_ROWS_NIBBLES) ? 1 : 0;
        K1Setup su; bool fits = false;
        bool can = merge && (int)merged.size() < K1V3_MAX_BANDS;
        if (can) {
            if (pairs) { rc = check_pairs("kbbq_accumulate_bands_dev", b.nrows, S2); if (rc) return rc; }
            rc = accumulate_rows(c, "kbbq_accumulate_bands_dev", b.d_seq, b.d_cseq, b.d_qual, b.d_meta, b.nrows, b.pitch, pairs, R, S2, minscore,
                                 dinuc_minscore, b.d_seg, d_tables, &fits, pairs ? 0 : b.S_band, pairs ? 0 : b.S_min, nib,
                                 (b.flags & KBBQ_ROWS_TWINS) ? 1 : 0, &su, (b.flags & KBBQ_ROWS_ERRBIT) ? 1 : 0);
            if (rc) return rc;
            can = fits && !su.kj && (nib_of_merge < 0 || nib_of_merge == nib);
        }
        if (can) { nib_of_merge = nib; merged.push_back(i); setups.push_back(su); }
        else alone.push_back(i);
    }
    // at least two bands, no more than one 16-wave workgroup per CU and read group gives each of them: ONE launch; anything else goes alone
    const int G = std::max(1, c->cus / std::max(R, 1));
    if (merged.size() < 2 || (int)merged.size() > G) { for (int i : merged) alone.push_back(i); merged.clear(); }
    for (int i : alone) {
        int rc = band_accumulate_alone(c, bands[i], R, S2, minscore, dinuc_minscore, d_tables);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    if (merged.empty()) return KBBQ_OK;
    // a band's share of the workgroups follows its work: chunks to bin plus a per-row term (a 64-row block pays the sidecar
    // -> row address -> first chunk latency whatever its width: narrow rows run at half the rate of wide ones) ...
    constexpr double row_cost = 1.25;
    // ... and a chunk of a WIDE row costs more than a chunk of a narrow one (larger tables to zero and flush, 8 instead of 16 copies
    // of the context table, more cycle columns for the same lanes): with equal cost per chunk the widest band of BASELINE config 5
    // ended 25 % after the narrowest (KBBQ_K1_BANDS_DBG=1 prints every band's workgroup end times): + 1 % per chunk of row width
    constexpr double slope = 0.01;
    constexpr double dn8_cost = 1.06;                     // a band on 8 copies of the context table: twice the same-address atomics there
    K1BandsParams t;
    memset(&t, 0, sizeof t);
    t.nbands = (int)merged.size();
    std::vector<double> weight; std::vector<int64_t> cap; std::vector<int> share;
    size_t lds = 0;
    for (const K1Setup& su : setups) {
        weight.push_back((double)su.q.nreads * (su.q.cpr + row_cost) * (1.0 + slope * su.q.cpr) * (su.dn == K1V3_DNREP ? 1.0 : dn8_cost));
        cap.push_back(std::max<int64_t>(1, k1_iters(su.q)));
        lds = std::max(lds, su.lds);
    }
    share_workgroups(weight, cap, G, share);
    int run = 0;
    for (size_t j = 0; j < setups.size(); ++j) {
        t.wg_start[j] = run; run += share[j];
        t.dn[j] = setups[j].dn; t.band[j] = setups[j].q;
    }
    t.wg_start[setups.size()] = run;
    unsigned long long* dbg = nullptr;                    // KBBQ_K1_BANDS_DBG=1: when did every band's workgroups start and end?
    if (getenv("KBBQ_K1_BANDS_DBG")) { HIPCHK(hipMalloc((void**)&dbg, sizeof(unsigned long long) * 2 * (size_t)run)); t.dbg = dbg; }
    int rc = launch_lds(c, 0, k1_kernel(K1_BANDS, k1_split(setups[0].q), 0, nib_of_merge, 0), dim3((unsigned)run, (unsigned)R, 1),
                        dim3(K1V3_THREADS), lds, &t);
    if (rc) return rc;
    if (dbg) {
        std::vector<unsigned long long> h(2 * (size_t)run);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(h.data(), dbg, h.size() * sizeof h[0], hipMemcpyDeviceToHost));
        (void)hipFree(dbg);
        unsigned long long t0 = ~0ull;
        for (int w = 0; w < run; ++w) t0 = std::min(t0, h[(size_t)w]);
        for (int j = 0; j < t.nbands; ++j) {
            unsigned long long s1 = 0, e0 = ~0ull, e1 = 0;
            for (int w = t.wg_start[j]; w < t.wg_start[j + 1]; ++w) {
                s1 = std::max(s1, h[(size_t)w] - t0); e0 = std::min(e0, h[(size_t)run + w] - t0); e1 = std::max(e1, h[(size_t)run + w] - t0);
            }
            fprintf(stderr, "[k1v3_bands] band %d pitch %3d rows %9lld: %3d workgroups, last start %7.1f us, ends %7.1f .. %7.1f us\n", j, t.band[j].pitch,
                    (long long)t.band[j].nreads, t.wg_start[j + 1] - t.wg_start[j], s1 / 100.0, e0 / 100.0, e1 / 100.0);
        }
    }
    return KBBQ_OK;
}

static int band_apply_alone(kbbq_ctx* c, const kbbq_band& b, int R, int S2, int minscore, const void* d_lut_blob)
{
    if (b.flags || b.d_seg)
        return kbbq_apply_rows_dev(c, b.d_seq, b.d_qual, b.d_meta, b.nrows, b.pitch, b.flags, R, S2, minscore, d_lut_blob, b.d_pair_lut,
                                   b.d_seg, b.d_perm, b.d_out);
    return kbbq_apply_dev(c, b.d_seq, b.d_qual, b.d_meta, b.nrows, b.pitch, R, KQ, S2, minscore, d_lut_blob, KBBQ_APPLY_FAST, b.d_out);
}

int kbbq_apply_bands_dev(kbbq_ctx* c, const kbbq_band* bands, int nbands, int R, int S2, int minscore, const void* d_lut_blob)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbands < 0 || (nbands > 0 && !bands) || !d_lut_blob) return fail(KBBQ_E_ARG, "kbbq_apply_bands_dev: bad argument");
    if (R <= 0 || R > 32767 || S2 <= 0 || (S2 & 1) || S2 > 65534 || minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "kbbq_apply_bands_dev: bad shape");
    // the merged kernel (k2t_bands) takes what the short-lived kernel takes (k2_tile_serves) of one-read-per-row 4-bit planes
    // with one read group; the rest goes band by band.
    // Unlike apply_rows, the LUT's cycle width is min(pitch, S2) whatever KBBQ_K2_ROWLUT says, only R == 1 merges (not rows
    // grouped by read group), and pointers and alignment are tested here: a band that fails them goes alone and is reported there.
    std::vector<int> merged, alone;
    for (int i = 0; i < nbands; ++i) {
        const kbbq_band& b = bands[i];
        if (b.nrows == 0) continue;
        int rc = layout_flags_ok("kbbq_apply_bands_dev", b.flags, true);           // (k2t_bands takes b.flags == KBBQ_ROWS_NIBBLES alone)
        if (rc) return rc;
        const int Sb = std::min(b.pitch, S2);
        const bool can = (int)merged.size() < K2T_MAX_BANDS && R == 1
                         && b.flags == KBBQ_ROWS_NIBBLES && !b.d_seg && !b.d_perm && b.pitch > 0 && !(b.pitch & 15)
                         && k2_tile_serves(c, 0, 1, R, false, b.pitch / 16, (size_t)(33 + KQ) * full_lut_row_bytes(Sb))
                         && !(((uintptr_t)b.d_seq | (uintptr_t)b.d_qual | (uintptr_t)b.d_out) & 15) && b.d_seq && b.d_qual && b.d_meta && b.d_out;
        (can ? merged : alone).push_back(i);
    }
    if (merged.size() < 2) { for (int i : merged) alone.push_back(i); merged.clear(); }
    for (int i : alone) {
        int rc = band_apply_alone(c, bands[i], R, S2, minscore, d_lut_blob);
        if (rc) return rc;
    }
    if (merged.empty()) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    // every band's LUT, narrowed to the columns rows of its pitch can reach, side by side in the context's scratch
    std::vector<size_t> lut_off; size_t need = 0;
    for (int i : merged) { lut_off.push_back(need); need += ((size_t)R * (33 + KQ) * full_lut_row_bytes(std::min(bands[i].pitch, S2)) + 255) & ~(size_t)255; }
    int rc = grow_scratch(c, c->rowlut, need);
    if (rc) return rc;
    K2tBandsParams t;
    memset(&t, 0, sizeof t);
    t.nbands = (int)merged.size();
    const int64_t per_wg = (int64_t)(K2T_THREADS / 64) * 64 * K2T_STEPS;
    int64_t run = 0; size_t lds = 0;
    for (size_t k = 0; k < merged.size(); ++k) {
        const kbbq_band& b = bands[merged[k]];
        const int Sb = std::min(b.pitch, S2);
        K2v3Params rows = k2v3_params(c, b.d_seq, b.d_qual, b.d_meta, b.nrows, b.pitch, 0, R, KQ, S2, Sb, minscore, d_lut_blob, nullptr, nullptr, nullptr, b.d_out);
        rows.full = fill_row_lut(c, d_lut_blob, R, KQ, S2, Sb, minscore, reinterpret_cast<char*>(c->rowlut.p) + lut_off[k]);
        const K2tParams& q = t.band[k] = k2t_params(rows);
        lds = std::max(lds, (size_t)q.lut_bytes);
        t.wg_start[k] = (int)run;
        run += (q.nchunks + per_wg - 1) / per_wg;
        if (run > 0x7FFFFFFF) return fail(KBBQ_E_ARG, "kbbq_apply_bands_dev: too many workgroups");
    }
    t.wg_start[merged.size()] = (int)run;
    return launch_lds(c, 1, LDS_KERNELS[LK_K2T_BANDS], dim3((unsigned)run), dim3(K2T_THREADS), lds, &t);
}

int kbbq_meta_stats_dev(kbbq_ctx* c, const uint32_t* d_meta, int64_t nreads, int32_t* h_stats8)
{
    if (!c || !h_stats8) return fail(KBBQ_E_ARG, "kbbq_meta_stats_dev: NULL argument");
    if (nreads < 0) return fail(KBBQ_E_ARG, "kbbq_meta_stats_dev: nreads < 0");
    static const int init[K7_NSTATS] = {0x7FFFFFFF, 0, 0, 0, 0, 0, 0, 0};
    memcpy(h_stats8, init, sizeof init);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_stats) HIPCHK(hipMalloc((void**)&c->d_stats, sizeof init));
    HIPCHK(hipMemcpyAsync(c->d_stats, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    MetaStatsParams p; p.meta = d_meta; p.n = nreads; p.stats = c->d_stats;
    const int64_t npairs = (nreads + 1) / 2;
    int gx = (int)std::min<int64_t>((npairs + 255) / 256, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(k7_meta_stats, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_stats8, c->d_stats, sizeof init, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

size_t kbbq_group_rows_work_bytes(int64_t nrows, int R)
{
    const int64_t nblocks = (nrows + K7_SORT_ROWS - 1) / K7_SORT_ROWS;
    return (size_t)std::max<int64_t>(nblocks, 1) * (size_t)std::max(R, 1) * sizeof(u32);
}

int kbbq_group_rows_dev(kbbq_ctx* c, const uint32_t* d_meta, int64_t nrows, int pairs, int R, void* d_work,
                        int64_t* d_perm, int64_t* d_seg)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nrows < 0 || nrows >= (1ll << 32)) return fail(KBBQ_E_ARG, "kbbq_group_rows_dev: nrows out of range");
    if (R <= 0 || R > K7_SORT_MAXR) return fail(KBBQ_E_ARG, "kbbq_group_rows_dev: 1 <= R <= %d (got %d)", K7_SORT_MAXR, R);
    if (!d_meta || !d_work || !d_perm || !d_seg) return fail(KBBQ_E_ARG, "kbbq_group_rows_dev: NULL pointer");
    HIPCHK(hipSetDevice(c->device));
    if (nrows == 0) { HIPCHK(hipMemsetAsync(d_seg, 0, (size_t)(R + 1) * 8, c->stream)); return KBBQ_OK; }
    RgSortParams p;
    p.meta = d_meta; p.nrows = nrows; p.pairs = pairs ? 1 : 0; p.R = R;
    p.nblocks = (nrows + K7_SORT_ROWS - 1) / K7_SORT_ROWS;
    p.hist = reinterpret_cast<u32*>(d_work); p.perm = reinterpret_cast<long long*>(d_perm); p.status = c->d_status;
    hipLaunchKernelGGL(k7_rg_sort<false>, dim3((unsigned)p.nblocks), dim3(K7_SORT_THREADS), 0, c->stream, p);
    RgScanParams s;
    s.hist = p.hist; s.count = p.nblocks * R; s.nblocks = p.nblocks; s.R = R; s.nrows = nrows; s.seg = reinterpret_cast<long long*>(d_seg);
    hipLaunchKernelGGL(k7_rg_scan, dim3(1), dim3(1024), 0, c->stream, s);
    hipLaunchKernelGGL(k7_rg_sort<true>, dim3((unsigned)p.nblocks), dim3(K7_SORT_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_lay_out_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual, const uint32_t* d_meta,
                     int64_t nreads, int pitch, int flags, int S2, const int64_t* d_perm,
                     uint8_t* d_lseq, uint8_t* d_lcseq, uint8_t* d_lqual, uint32_t* d_lmeta)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = layout_flags_ok("kbbq_lay_out_dev", flags, true);
    if (rc) return rc;
    const int pairs = (flags & KBBQ_ROWS_PAIRS) ? 1 : 0, nib = (flags & KBBQ_ROWS_NIBBLES) ? 1 : 0, errbit = (flags & KBBQ_ROWS_ERRBIT) ? 1 : 0;
    if (errbit && (!d_cseq || (pair_pitch(S2) != 16 * 19 && pair_pitch(S2) != 16 * 13)))
        return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: KBBQ_ROWS_ERRBIT needs the corrected reads and mate-pair rows of 19 or 13 chunks");
    rc = check_planes("kbbq_lay_out_dev", nreads, pitch, d_seq, d_cseq, d_qual);
    if (rc) return rc;
    if (!d_seq || !d_qual || !d_meta || !d_lseq || !d_lqual || !d_lmeta || (d_cseq && !d_lcseq && !errbit)) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: NULL pointer");
    if (((uintptr_t)d_lseq | (uintptr_t)d_lcseq | (uintptr_t)d_lqual) & 15) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: planes must be 16-byte aligned");
    if (pairs) {
        rc = check_pairs("kbbq_lay_out_dev", (nreads + 1) / 2, S2);
        if (rc) return rc;
        if ((nreads & 1) && !(flags & KBBQ_ROWS_TWINS)) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: mate-pair rows need an even number of reads");
        if (pitch < S2 / 2) return fail(KBBQ_E_ARG, "kbbq_lay_out_dev: pitch %d < read length %d", pitch, S2 / 2);
    }
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    LayOutParams p;
    p.src[0] = d_seq; p.src[1] = d_cseq; p.src[2] = d_qual; p.dst[0] = d_lseq; p.dst[1] = d_lcseq; p.dst[2] = d_lqual;
    p.meta = d_meta; p.dmeta = d_lmeta; p.perm = reinterpret_cast<const long long*>(d_perm);
    p.nrows = pairs ? (nreads + 1) / 2 : nreads; p.nsrc = nreads; p.pitch = pitch; p.dpitch = pairs ? pair_pitch(S2) : pitch; p.S = pairs ? S2 / 2 : 0;
    p.pairs = pairs; p.nib = nib; p.errbit = errbit; p.status = c->d_status;
    const int rpb7 = (p.dpitch / 16) <= 256 ? 256 / (p.dpitch / 16) : 1;      // destination rows per workgroup iteration
    const int gx = bounded_grid((p.nrows + rpb7 - 1) / rpb7, c, 256);
    p.parts = K7_FRONTS;
    hipLaunchKernelGGL(k7_lay_out, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_tables_add_dev(kbbq_ctx* c, int64_t* d_dst, const int64_t* d_src, size_t n)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (n && (!d_dst || !d_src)) return fail(KBBQ_E_ARG, "kbbq_tables_add_dev: NULL pointer");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    AddTablesParams p; p.dst = (long long*)d_dst; p.src = (const long long*)d_src; p.n = (long long)n;
    int gx = (int)std::min<size_t>((n + 255) / 256, (size_t)c->cus * 8);
    hipLaunchKernelGGL(k7_add_tables, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_unpack_nibbles_dev(kbbq_ctx* c, const uint8_t* d_nib, int64_t nbases, uint8_t* d_chars)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbases < 0 || (nbases & 15) || ((uintptr_t)d_nib & 7) || ((uintptr_t)d_chars & 15)) return fail(KBBQ_E_ARG, "kbbq_unpack_nibbles_dev: bad size or alignment");
    if (nbases == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    UnNibParams p; p.src = d_nib; p.dst = d_chars; p.nchunks = nbases / 16;
    int gx = (int)std::min<int64_t>((p.nchunks + 255) / 256, (int64_t)c->cus * 16);
    hipLaunchKernelGGL(k7_unpack_nibbles, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// K4's view of a batch of aligned reads; skipmask == NULL: bit 7 of a reference byte is its site flag; skip == NULL: ONE plane of
// flags (err)
static K4Params k4_params(kbbq_ctx* c, const uint8_t* d_seq, const uint32_t* d_len, int64_t nreads, int pitch, const int64_t* d_ref_start,
                          const int32_t* d_ref_len, const uint32_t* d_cig_off, const uint32_t* d_cig_n, const uint32_t* d_cigar,
                          const uint8_t* d_genome, const uint8_t* d_skipmask, int64_t genome_len, const uint8_t* d_flip, uint8_t* d_err,
                          uint8_t* d_skip)
{
    K4Params p;
    p.seq = d_seq; p.len = d_len; p.nreads = nreads; p.pitch = pitch;
    p.ref_start = (const long long*)d_ref_start; p.ref_len = d_ref_len;
    p.cig_off = d_cig_off; p.cig_n = d_cig_n; p.cigar = d_cigar;
    p.genome = d_genome; p.skipmask = d_skipmask; p.genome_len = genome_len; p.flip = d_flip; p.err = d_err; p.skip = d_skip;
    p.status = c->d_status;
    return p;
}

// the first four operations of every read inline, one 32-byte record per read (context-owned scratch); with aflags_out also
// the classification kbbq_tally_aligned_dev needs (K4RecParams)
static int k4_records(kbbq_ctx* c, const K4Params& p, const u32* aflags_in, u32* aflags_out, u32* rows, u32* nrows, int pitch)
{
    int rc = grow_scratch(c, c->ops4, (size_t)p.nreads * sizeof(K4Rec));
    if (rc) return rc;
    K4RecParams ip; ip.len = p.len; ip.ref_len = p.ref_len; ip.cig_off = p.cig_off; ip.cig_n = p.cig_n; ip.cigar = p.cigar;
    ip.nreads = p.nreads; ip.recs = (K4Rec*)c->ops4.p;
    ip.aflags_in = aflags_in; ip.aflags_out = aflags_out; ip.rows = rows; ip.nrows = nrows;
    ip.ref_start = p.ref_start; ip.genome_len = p.genome_len; ip.pitch = pitch;
    int gi = (int)std::min<int64_t>((p.nreads + 255) / 256, (int64_t)c->cus * 16);
    hipLaunchKernelGGL(k4_read_records, dim3((unsigned)std::max(gi, 1)), dim3(256), 0, c->stream, ip);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// ---- K4 / K5: benchmark path --------------------------------------------
int kbbq_find_errors_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint32_t* d_len, int64_t nreads, int pitch,
                         const int64_t* d_ref_start, const int32_t* d_ref_len,
                         const uint32_t* d_cig_off, const uint32_t* d_cig_n, const uint32_t* d_cigar,
                         const uint8_t* d_genome, const uint8_t* d_skipmask, int64_t genome_len,
                         const uint8_t* d_flip, uint8_t* d_err, uint8_t* d_skip)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nreads < 0 || pitch <= 0 || (pitch & 15) || genome_len < 0) return fail(KBBQ_E_ARG, "kbbq_find_errors_dev: bad nreads/pitch/genome_len");
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    const K4Params p = k4_params(c, d_seq, d_len, nreads, pitch, d_ref_start, d_ref_len, d_cig_off, d_cig_n, d_cigar, d_genome, d_skipmask,
                                 genome_len, d_flip, d_err, d_skip);
    if (((uintptr_t)d_seq | (uintptr_t)d_err | (uintptr_t)d_skip) & 15)
        return fail(KBBQ_E_ARG, "kbbq_find_errors_dev: planes must be 16-byte aligned");
    const int rpb4 = (pitch / 16) <= 256 ? 256 / (pitch / 16) : 1;              // reads per workgroup iteration
    const int gx = bounded_grid((nreads + rpb4 - 1) / rpb4, c, 64);
    int rc4 = k4_records(c, p, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc4) return rc4;
    K4v2Params q; q.base = p; q.recs = (const K4Rec*)c->ops4.p; q.idle16 = reinterpret_cast<const uint8_t*>(c->d_status);
    q.rows = nullptr; q.nrows = nullptr;
    if (d_skipmask) hipLaunchKernelGGL(k4v2_find_errors<false>, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, q);
    else hipLaunchKernelGGL(k4v2_find_errors<true>, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, q);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_canonical_reads_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_err,
                             const uint8_t* d_skip, const uint32_t* d_len, const uint32_t* d_clip,
                             const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads, int pitch, int S,
                             int minscore, int dinuc_minscore, uint8_t* d_out_seq, uint8_t* d_out_cseq,
                             uint8_t* d_out_qual, uint32_t* d_out_meta)
{
    return kbbq_canonical_reads_rows_dev(c, d_seq, d_oq, d_err, d_skip, d_len, d_clip, d_trim, d_flags, nreads, pitch, S,
                                         minscore, dinuc_minscore, 0, d_out_seq, d_out_cseq, d_out_qual, d_out_meta);
}

int kbbq_canonical_reads_rows_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_err,
                                  const uint8_t* d_skip, const uint32_t* d_len, const uint32_t* d_clip,
                                  const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads, int pitch, int S,
                                  int minscore, int dinuc_minscore, int layout, uint8_t* d_out_seq, uint8_t* d_out_cseq,
                                  uint8_t* d_out_qual, uint32_t* d_out_meta)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (layout & KBBQ_ROWS_ERRBIT) return fail(KBBQ_E_ARG, "kbbq_canonical_reads_rows_dev: layout flags 0x%x: KBBQ_ROWS_ERRBIT describes mate-pair rows; the output is one read per row", layout);
    if (layout & ~KBBQ_ROWS_NIBBLES) return fail(KBBQ_E_ARG, "kbbq_canonical_reads_rows_dev: the output is one read per row (layout 0 or KBBQ_ROWS_NIBBLES)");
    if (nreads < 0 || pitch <= 0 || (pitch & 15) || S <= 0 || S > pitch || S > 65535)
        return fail(KBBQ_E_ARG, "kbbq_canonical_reads_dev: bad nreads/pitch/S");
    if (minscore < 0 || minscore > 94 || dinuc_minscore < 0 || dinuc_minscore > 94)
        return fail(KBBQ_E_ARG, "kbbq_canonical_reads_dev: minscore out of range");
    if (nreads == 0) return KBBQ_OK;
    if (!d_seq || !d_oq || !d_err) return fail(KBBQ_E_ARG, "kbbq_canonical_reads_dev: NULL plane");
    if (((uintptr_t)d_seq | (uintptr_t)d_oq | (uintptr_t)d_err | (uintptr_t)d_skip | (uintptr_t)d_out_seq
         | (uintptr_t)d_out_cseq | (uintptr_t)d_out_qual) & 15)
        return fail(KBBQ_E_ARG, "kbbq_canonical_reads_dev: planes must be 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    K6Params p;
    p.seq = d_seq; p.oq = d_oq; p.err = d_err; p.skip = d_skip; p.len = d_len; p.clip = d_clip; p.trim = d_trim;
    p.flags = d_flags; p.nreads = nreads; p.pitch = pitch; p.S = S;
    p.qlo = 33u + (u32)minscore; p.dlo = 33u + (u32)dinuc_minscore;
    p.out_seq = d_out_seq; p.out_cseq = d_out_cseq; p.out_qual = d_out_qual; p.out_meta = d_out_meta;
    p.status = c->d_status;
    const int rpb6 = (pitch / 16) <= 256 ? 256 / (pitch / 16) : 1;
    const int gx = bounded_grid((nreads + rpb6 - 1) / rpb6, c, 64);
    if (layout & KBBQ_ROWS_NIBBLES) hipLaunchKernelGGL(k6_canonical_reads<true>, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL(k6_canonical_reads<false>, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// K6 fused into K1 (k1v3_aligned): the BAM-sourced tally straight from the reads as aligned -- 3 B/base read (sequence, OQ,
// K4's plane of flags), nothing written but the count tables; kbbq_canonical_reads_rows_dev + kbbq_accumulate_rows_dev moved
// 3 + 2 + 2 B/base for the same tables.
// d_genome / d_g0 non-NULL: the REF form (k1v3_aligned_ref) -- reads whose d_flags word has bit 2 set are compared with the
// reference by the kernel itself (kbbq_tally_aligned_dev)
static int accumulate_aligned(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_flagplane,
                              const uint32_t* d_clip, const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads,
                              int pitch, int S, int R, int minscore, int dinuc_minscore, int64_t* d_tables,
                              const uint8_t* d_genome, const int64_t* d_g0, bool dry_run = false)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    int rc = check_planes("kbbq_accumulate_aligned_dev", nreads, pitch, d_seq, d_oq, d_flagplane);
    if (rc) return rc;
    if (S <= 0 || S > pitch || S > 32767 || pitch != ((S + 15) & ~15)) return fail(KBBQ_E_ARG, "kbbq_accumulate_aligned_dev: rows of S = %d bases have pitch %d (got %d)", S, (S + 15) & ~15, pitch);
    if (R <= 0 || R > 32767) return fail(KBBQ_E_ARG, "kbbq_accumulate_aligned_dev: R out of range (%d)", R);
    if (minscore < 0 || minscore > KQ - 1 || dinuc_minscore < 0 || dinuc_minscore > 94) return fail(KBBQ_E_ARG, "kbbq_accumulate_aligned_dev: minscore out of range");
    if (nreads == 0) return KBBQ_OK;
    if (!d_seq || !d_oq || !d_flagplane || !d_clip || !d_trim || !d_flags || !d_tables) return fail(KBBQ_E_ARG, "kbbq_accumulate_aligned_dev: NULL pointer");
    if (S < 32) return fail(KBBQ_E_LUT, "kbbq_accumulate_aligned_dev: reads of %d bases (< 32) are tallied through kbbq_canonical_reads_rows_dev", S);
    HIPCHK(hipSetDevice(c->device));
    K1Setup su;
    K1v3Params& q = su.q;
    memset(&q, 0, sizeof q);
    q.seq = d_seq; q.cseq = d_flagplane; q.qual = d_oq; q.meta = nullptr;
    q.aflags = d_flags; q.aclip = d_clip; q.atrim = d_trim;
    q.genome = d_genome; q.ag0 = reinterpret_cast<const long long*>(d_g0);
    q.nreads = nreads; q.pitch = pitch; q.cpr = pitch / 16; q.cpr_magic = magic_for(q.cpr);
    q.R = R; q.S = S; q.gS2 = 2 * S; q.minscore = minscore; q.type_minscore = dinuc_minscore;
    q.qlo_m1 = 32u + (u32)minscore; q.dlo = 33u + (u32)dinuc_minscore;
    q.nrows = KQ + 1 - minscore;
    q.maxlen = S; q.gap = 0; q.twins = 0; q.seg = nullptr;
    q.tables = reinterpret_cast<u64*>(d_tables); q.status = c->d_status;
    // LDS geometry as accumulate_rows: 3S words per cycle row (every read has length S: [0, S) read 1, [S, 2S) read 2 mirrored);
    // 16 copies of the context table, or 8 when that does not fit.
    // minlen = S: the flush walks columns [0, 2S) only -- the words behind them take the uncounted bytes in front of a read's
    // first aligned base (kernel comment) and are never read
    for (int copies : {K1V3_DNREP, 8})
        if (k1_geometry(q, c, copies, 0, S)) { su.dn = copies; break; }
    if (!su.dn) return fail(KBBQ_E_LUT, "kbbq_accumulate_aligned_dev: %d-base reads with minscore %d do not fit the LDS tables; tally through kbbq_canonical_reads_rows_dev", S, minscore);
    if (dry_run) return KBBQ_OK;                      // the caller only asked whether this shape is served
    su.lds = k1_lds_plan(q, su.dn, c);                // trash rows and copies of the cycle table, as accumulate_rows
    return launch_k1(c, d_genome ? K1_ALIGNED_REF : K1_ALIGNED, su, 0);
}

int kbbq_accumulate_aligned_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_flagplane,
                                const uint32_t* d_clip, const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads,
                                int pitch, int S, int R, int minscore, int dinuc_minscore, int64_t* d_tables)
{
    return accumulate_aligned(c, d_seq, d_oq, d_flagplane, d_clip, d_trim, d_flags, nreads, pitch, S, R, minscore, dinuc_minscore,
                              d_tables, nullptr, nullptr);
}

// The whole BAM-sourced tally (gatk/bqsr.py:52-123: find_read_errors per read, then the covariate counts) with ONE pass over
// the reads for everything but the reads K4 has to walk.  kbbq_find_errors_dev + kbbq_accumulate_aligned_dev move read bytes
// and the reference in, a plane of flags out and read bytes, flags and OQ in again: 6 B/base.  Here k4_read_records sorts the
// reads: one M / = / X operation over all bases, every 16-byte reference window readable -> the tally kernel compares read and
// reference itself (k1v3_aligned_ref: read bytes, OQ, reference window = 3 B/base); every other read (indels, clips in the
// CIGAR, anything odd) is listed, k4v2_find_errors writes the rows of d_flagplane of just those reads, and the tally kernel
// reads them there.  d_flagplane: [nreads, pitch] scratch of the caller's, contents on entry irrelevant.  The reference must
// carry the site flags in bit 7 (d_skipmask == NULL in kbbq_find_errors_dev's terms).  Every read has S bases (d_len[i] == S
// is the caller's promise, as for kbbq_accumulate_aligned_dev).  Counts are what kbbq_find_errors_dev (no flip) followed by
// kbbq_accumulate_aligned_dev count; the same statuses are raised (KBBQ_E_LUT: use kbbq_canonical_reads_rows_dev).
int kbbq_tally_aligned_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_oq, const uint32_t* d_len, int64_t nreads,
                           int pitch, int S, const int64_t* d_ref_start, const int32_t* d_ref_len,
                           const uint32_t* d_cig_off, const uint32_t* d_cig_n, const uint32_t* d_cigar,
                           const uint8_t* d_genome, int64_t genome_len,
                           const uint32_t* d_clip, const uint32_t* d_trim, const uint32_t* d_flags,
                           uint8_t* d_flagplane, int R, int minscore, int dinuc_minscore, int64_t* d_tables)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nreads < 0 || nreads > 0xFFFFFFFFll || pitch <= 0 || (pitch & 15) || genome_len < 0) return fail(KBBQ_E_ARG, "kbbq_tally_aligned_dev: bad nreads/pitch/genome_len");
    if (nreads == 0) return KBBQ_OK;
    if (!d_seq || !d_oq || !d_len || !d_ref_start || !d_ref_len || !d_cig_off || !d_cig_n || !d_cigar || !d_genome || !d_clip || !d_trim
        || !d_flags || !d_flagplane || !d_tables) return fail(KBBQ_E_ARG, "kbbq_tally_aligned_dev: NULL pointer");
    if (((uintptr_t)d_seq | (uintptr_t)d_oq | (uintptr_t)d_flagplane) & 15) return fail(KBBQ_E_ARG, "kbbq_tally_aligned_dev: planes must be 16-byte aligned");
    // what the tally kernel refuses it refuses before anything is launched (same checks, same codes)
    if (S <= 0 || S > pitch || S > 32767 || pitch != ((S + 15) & ~15)) return fail(KBBQ_E_ARG, "kbbq_tally_aligned_dev: rows of S = %d bases have pitch %d (got %d)", S, (S + 15) & ~15, pitch);
    if (S < 32) return fail(KBBQ_E_LUT, "kbbq_tally_aligned_dev: reads of %d bases (< 32) are tallied through kbbq_canonical_reads_rows_dev", S);
    int rc = accumulate_aligned(c, d_seq, d_oq, d_flagplane, d_clip, d_trim, d_flags, nreads, pitch, S, R, minscore, dinuc_minscore,
                                d_tables, d_genome, d_ref_start, true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = grow_scratch(c, c->tally, 16 + 2 * (size_t)nreads * sizeof(u32));
    if (rc) return rc;
    u32* count = reinterpret_cast<u32*>(c->tally.p);
    u32* aflags2 = count + 4;
    u32* rows = aflags2 + nreads;
    HIPCHK(hipMemsetAsync(count, 0, 16, c->stream));
    const K4Params p = k4_params(c, d_seq, d_len, nreads, pitch, d_ref_start, d_ref_len, d_cig_off, d_cig_n, d_cigar, d_genome, nullptr,
                                 genome_len, nullptr, d_flagplane, nullptr);
    rc = k4_records(c, p, d_flags, aflags2, rows, count, pitch);
    if (rc) return rc;
    {   // K4 over the listed reads only: their number is on the device, the grid is sized for a share of the reads (a workgroup
        // beyond the list's end finds nothing to do)
        const int rpb4 = (pitch / 16) <= 256 ? 256 / (pitch / 16) : 1;
        const int gx = bounded_grid(((nreads + TALLY_K4_SHARE - 1) / TALLY_K4_SHARE + rpb4 - 1) / rpb4, c, 64);
        K4v2Params q; q.base = p; q.recs = (const K4Rec*)c->ops4.p; q.idle16 = reinterpret_cast<const uint8_t*>(c->d_status);
        q.rows = rows; q.nrows = count;
        hipLaunchKernelGGL(k4v2_find_errors<true>, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, q);
        HIPCHK(hipGetLastError());
    }
    return accumulate_aligned(c, d_seq, d_oq, d_flagplane, d_clip, d_trim, aflags2, nreads, pitch, S, R, minscore, dinuc_minscore,
                              d_tables, d_genome, d_ref_start);
}

int kbbq_count_q_dev(kbbq_ctx* c, const uint8_t* d_qual, const uint8_t* d_err, const uint8_t* d_skip,
                     const uint32_t* d_len, int64_t nreads, int pitch, int qoffset, int64_t* d_counts512)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_qual || !d_err) return fail(KBBQ_E_ARG, "kbbq_count_q_dev: NULL plane");
    int rc = check_planes("kbbq_count_q_dev", nreads, pitch, d_qual, d_err, d_skip);
    if (rc) return rc;
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K5Params p;
    p.qual = d_qual; p.err = d_err; p.skip = d_skip; p.len = d_len; p.nreads = nreads; p.pitch = pitch;
    p.cpr = pitch / 16; p.cpr_magic = magic_for(p.cpr); p.qoffset = qoffset;
    p.counts = reinterpret_cast<u64*>(d_counts512); p.status = c->d_status;
    const int64_t nchunks = nreads * p.cpr;
    const int gx = bounded_grid((nchunks + 255) / 256, c, 64);
    hipLaunchKernelGGL(k5_count_q, dim3((unsigned)std::max(gx, 1)), dim3(256), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_flag_confusion_dev(kbbq_ctx* c, const uint8_t* d_qual, const uint8_t* d_truth, const uint8_t* d_kflags,
                            const uint32_t* d_len, int64_t nreads, int pitch, int qoffset, int64_t* d_counts1536)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_qual || !d_truth || !d_kflags) return fail(KBBQ_E_ARG, "kbbq_flag_confusion_dev: NULL plane");
    if (!d_len || !d_counts1536) return fail(KBBQ_E_ARG, "kbbq_flag_confusion_dev: NULL d_len or d_counts1536");
    int rc = check_planes("kbbq_flag_confusion_dev", nreads, pitch, d_qual, d_truth, d_kflags);
    if (rc) return rc;
    // byte - qoffset indexes 257 bins: a negative offset would carry it past them
    if (qoffset < 0 || qoffset > 255) return fail(KBBQ_E_ARG, "kbbq_flag_confusion_dev: qoffset must be in 0..255, got %d", qoffset);
    // the kernel's LDS counters are 32 bits wide and flushed once: one increment per byte read at most
    if (nreads > (int64_t)(KBBQ_CONFUSION_MAX_BASES / (uint64_t)pitch))
        return fail(KBBQ_E_ARG, "kbbq_flag_confusion_dev: nreads * pitch = %lld * %d exceeds %llu bases per call (32-bit counters): "
                    "split the rows over several calls, which add into the same counts", (long long)nreads, pitch,
                    (unsigned long long)KBBQ_CONFUSION_MAX_BASES);
    if (nreads == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    K5JParams p;
    p.qual = d_qual; p.truth = d_truth; p.kflags = d_kflags; p.len = d_len; p.nreads = nreads; p.pitch = pitch;
    p.cpr = pitch / 16; p.qoffset = qoffset;
    p.counts = reinterpret_cast<u64*>(d_counts1536); p.status = c->d_status;
    const int64_t nchunks = nreads * p.cpr;
    const int gx = bounded_grid((nchunks + K5J_THREADS - 1) / K5J_THREADS, c, K5J_WG_PER_CU);
    hipLaunchKernelGGL(k5j_flag_confusion, dim3((unsigned)gx), dim3(K5J_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// ---- host-buffer entry points: stage, run, fetch -------------------------
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
};

// ---- host-buffer entry points: slabs of rows through page-locked staging -------------------------------------------------
// A caller's NumPy arrays are pageable memory: hipMemcpy from them goes through the runtime's own small staging buffers, one
// plane after the other, and the kernel starts when the last byte has arrived.  Here the rows travel in slabs: host threads
// copy slab k + 1 into a page-locked buffer while the copy engine uploads slab k and the kernel runs on slab k - 1 (apply: the
// new qualities of slab k - 2 come back meanwhile, PCIe being full duplex); device memory is two slabs, whatever the input's size.
static size_t stage_slab_rows(int pitch, int planes, int64_t nreads)
{
    const char* e = getenv("KBBQ_STAGE_MB");                       // staging bytes per slab (all planes), default 96 MB
    const size_t budget = (size_t)(e && atoi(e) > 0 ? atoi(e) : 96) << 20;
    size_t rows = budget / ((size_t)pitch * planes + 4);
    rows = std::max<size_t>(rows & ~(size_t)63, 64);
    return (size_t)std::min<int64_t>((int64_t)rows, std::max<int64_t>(nreads, 1));
}

static int stage_prepare(kbbq_ctx* c, size_t bytes)
{
    if (!c->stage_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->stage_stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&c->stage_down_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipEventCreateWithFlags(&c->stage_up[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->stage_used[b], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->stage_down[b], hipEventDisableTiming));
        }
    }
    if (c->stage_bytes < bytes) {
        HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipStreamSynchronize(c->stage_stream)); HIPCHK(hipStreamSynchronize(c->stage_down_stream));
        for (int b = 0; b < 2; ++b) {
            if (c->stage_host[b]) { (void)hipHostFree(c->stage_host[b]); c->stage_host[b] = nullptr; }
            if (c->stage_dev[b]) { (void)hipFree(c->stage_dev[b]); c->stage_dev[b] = nullptr; }
        }
        c->stage_bytes = 0;
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipHostMalloc(&c->stage_host[b], bytes, hipHostMallocDefault));
            HIPCHK(hipMalloc(&c->stage_dev[b], bytes));
        }
        c->stage_bytes = bytes;
    }
    return KBBQ_OK;
}

// copy `bytes` with all host threads (a slab is tens of MB: one thread moves ~10 GB/s, PCIe takes ~55)
static void threaded_copy(void* dst, const void* src, size_t bytes)
{
    const unsigned nt = kbbq_threads_for(bytes / 4);
    if (nt <= 1 || bytes < ((size_t)4 << 20)) { memcpy(dst, src, bytes); return; }
    const size_t per = ((bytes + nt - 1) / nt + 4095) & ~(size_t)4095;
    kbbq_parallel(nt, [&](unsigned t) {
        const size_t lo = std::min(bytes, (size_t)t * per), hi = std::min(bytes, lo + per);
        if (lo < hi) memcpy((char*)dst + lo, (const char*)src + lo, hi - lo);
    });
}

// Every exit of a pipelined run that leaves before its last slab -- a launch or a copy failed -- waits for what is still in
// flight: the staging buffers and their events belong to the context, and the next call's first two slabs do not wait on
// events of an earlier call.
static int stage_drain(kbbq_ctx* c, int rc)
{
    if (c->stage_stream) (void)hipStreamSynchronize(c->stage_stream);
    if (c->stage_down_stream) (void)hipStreamSynchronize(c->stage_down_stream);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// The status words hold the SMALLEST flagged read index of every kind over all launches since they were last read; slabs number
// their reads from 0, so after a pipelined run that flagged something the slabs are looked at again one by one (input errors
// are the rare case): the first slab that reproduces a status decides, its read index made file-wide (and handed back in
// *bad_read when the caller asks for it).
static int first_offender(kbbq_ctx* c, int64_t nreads, size_t slab, const std::function<int(int64_t, int64_t)>& run_slab,
                          int64_t* bad_read)
{
    for (int64_t lo = 0; lo < nreads; lo += (int64_t)slab) {
        const int64_t m = std::min<int64_t>((int64_t)slab, nreads - lo);
        int rc = run_slab(lo, m);
        if (rc) return rc;
        int64_t idx = -1;
        rc = kbbq_ctx_status(c, &idx);
        if (rc) {
            if (idx >= 0) {
                if (bad_read) *bad_read = lo + idx;
                const std::string what = g_err;
                const size_t colon = what.find(": ");
                return fail(rc, "read %lld%s", (long long)(lo + idx), colon == std::string::npos ? "" : what.c_str() + colon);
            }
            return rc;
        }
    }
    return KBBQ_OK;
}

// The pipelined run of a host-buffer entry point.  A slab holds the input planes `in`, the output plane (when `out` is given),
// then the meta words; `launch(d, plane, m)` runs the kernel on the m rows of device slab d, whose planes are `plane` bytes apart.
// Order of a slab k in buffers b = k & 1: [host] wait for slab k - 2 (with an output plane: for its download, whose rows then
// go to the caller -- everything of slab k - 2 on these buffers has finished, kernel included; without one: for its upload,
// and the upload stream waits for its kernel) -> host copy in -> upload (upload stream) -> kernel (launch stream, behind the
// upload's event) -> download (DOWNLOAD stream, behind the kernel's event).  Uploads and downloads are on different streams,
// so slab k + 1 goes up while slab k's kernel runs and slab k's (or k - 1's) output comes back: both directions of PCIe busy
// at once (with both on one in-order stream the order was strictly U k, K k, D k, U k + 1).
// `exact` (optional): the launch's kernel may answer KBBQ_E_LUT -- rows its fast form does not serve, no read named.  The entry
// point must not hand that to its caller: exact() switches `launch` to the form that decides (false: it already is that form)
// and the WHOLE input runs again -- such rows are the rare case -- so that clean rows with odd padding get their output and bad
// ones the reference's error with the read's index, here and slab by slab in first_offender.
// `see_meta` (optional): called with every slab's sidecar words (words, first read, count) as the slab is staged.
static int stage_run(kbbq_ctx* c, const char* who, std::initializer_list<const uint8_t*> in, const uint32_t* meta, uint8_t* out,
                     int64_t n, int pitch, const std::function<int(uint8_t*, size_t, int64_t)>& launch, int64_t* bad_read = nullptr,
                     const std::function<bool()>& exact = nullptr,
                     const std::function<void(const uint32_t*, int64_t, int64_t)>& see_meta = nullptr)
{
    const int planes = (int)in.size() + (out ? 1 : 0);
    const size_t slab = stage_slab_rows(pitch, planes, n);
    const size_t plane = slab * (size_t)pitch, o_out = in.size() * plane, o_meta = (size_t)planes * plane;
    int rc = stage_prepare(c, o_meta + slab * 4);
    if (rc) return rc;
    auto stage_in = [&](int b, int64_t lo, int64_t m) {
        uint8_t* h = (uint8_t*)c->stage_host[b];
        const size_t off = (size_t)lo * pitch, nb = (size_t)m * pitch;
        size_t at = 0;
        for (const uint8_t* p : in) { threaded_copy(h + at, p + off, nb); at += plane; }
        memcpy(h + o_meta, meta + lo, (size_t)m * 4);
        if (see_meta) see_meta(reinterpret_cast<const uint32_t*>(h + o_meta), lo, m);   // the slab's words, just copied: while earlier slabs upload and run
    };
    auto upload = [&](int b, int64_t m, hipStream_t st) -> int {        // the input planes, then the meta words
        HIPCHK(hipMemcpyAsync(c->stage_dev[b], c->stage_host[b], o_out, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((uint8_t*)c->stage_dev[b] + o_meta, (uint8_t*)c->stage_host[b] + o_meta, (size_t)m * 4, hipMemcpyHostToDevice, st));
        return KBBQ_OK;
    };
    struct Out { int64_t lo, m; };
    Out pending[2] = {{0, 0}, {0, 0}};                                   // downloads in flight, by buffer
    auto stage_out = [&](int b) -> int {                                 // wait for buffer b's download and hand its rows to the caller
        if (!pending[b].m) return KBBQ_OK;
        HIPCHK(hipEventSynchronize(c->stage_down[b]));
        threaded_copy(out + (size_t)pending[b].lo * pitch, (uint8_t*)c->stage_host[b] + o_out, (size_t)pending[b].m * pitch);
        pending[b].m = 0;
        return KBBQ_OK;
    };
    int64_t k = 0;
    auto pipelined = [&]() -> int {
        for (int64_t lo = 0; lo < n; lo += (int64_t)slab, ++k) {
            const int b = (int)(k & 1);
            const int64_t m = std::min<int64_t>((int64_t)slab, n - lo);
            int r2 = stage_out(b);                                            // slab k - 2 (same buffers): downloaded -> the caller's rows
            if (r2) return r2;
            if (!out && k >= 2) HIPCHK(hipEventSynchronize(c->stage_up[b]));  // the page-locked slab has been uploaded: free again
            stage_in(b, lo, m);
            if (!out && k >= 2) HIPCHK(hipStreamWaitEvent(c->stage_stream, c->stage_used[b], 0));   // the device slab's kernel has run
            r2 = upload(b, m, c->stage_stream);
            if (r2) return r2;
            HIPCHK(hipEventRecord(c->stage_up[b], c->stage_stream));
            HIPCHK(hipStreamWaitEvent(c->stream, c->stage_up[b], 0));
            r2 = launch((uint8_t*)c->stage_dev[b], plane, m);
            if (r2) return r2;
            HIPCHK(hipEventRecord(c->stage_used[b], c->stream));
            if (!out) continue;
            HIPCHK(hipStreamWaitEvent(c->stage_down_stream, c->stage_used[b], 0));
            HIPCHK(hipMemcpyAsync((uint8_t*)c->stage_host[b] + o_out, (uint8_t*)c->stage_dev[b] + o_out, (size_t)m * pitch, hipMemcpyDeviceToHost, c->stage_down_stream));
            HIPCHK(hipEventRecord(c->stage_down[b], c->stage_down_stream));
            pending[b] = {lo, m};
        }
        return KBBQ_OK;
    };
    for (int pass = 0; ; ++pass) {
        k = 0;
        rc = pipelined();
        if (rc) return stage_drain(c, rc);
        rc = kbbq_ctx_status(c, nullptr);
        if (rc != KBBQ_E_LUT || pass || !exact || !exact()) break;
        (void)stage_drain(c, rc);                                      // the fast run's last downloads: not the caller's rows
        pending[0].m = pending[1].m = 0;
    }
    if (rc == KBBQ_E_FULL) return stage_drain(c, rc);                  // the table, not a read: nothing to look for slab by slab
    if (rc) {
        // something was flagged: which read of the WHOLE input comes first?
        (void)stage_drain(c, rc);
        rc = first_offender(c, n, slab, [&](int64_t lo, int64_t m) {
            stage_in(0, lo, m);
            int r2 = upload(0, m, c->stream);
            return r2 ? r2 : launch((uint8_t*)c->stage_dev[0], plane, m);
        }, bad_read);
        return rc ? rc : fail(KBBQ_E_HIP, "%s: a status reported by the pipelined run did not reproduce slab by slab", who);
    }
    for (int b = 0; b < 2; ++b) { rc = stage_out((int)((k + b) & 1)); if (rc) return stage_drain(c, rc); }     // the older of the two first
    return KBBQ_OK;
}

int kbbq_accumulate(kbbq_ctx* c, const uint8_t* seq, const uint8_t* cseq, const uint8_t* qual,
                    const uint32_t* meta, int64_t nreads, int pitch, int R, int S2, int minscore,
                    int64_t* pos_errs, int64_t* pos_total, int64_t* dinuc_errs, int64_t* dinuc_total)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nreads < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "kbbq_accumulate: bad nreads/pitch");
    if (nreads > 0 && (!seq || !cseq || !qual || !meta)) return fail(KBBQ_E_ARG, "kbbq_accumulate: NULL plane");
    if (R <= 0 || S2 <= 0 || !pos_errs || !pos_total || !dinuc_errs || !dinuc_total) return fail(KBBQ_E_ARG, "kbbq_accumulate: bad tables");
    HIPCHK(hipSetDevice(c->device));
    const size_t npos = (size_t)R * KQ * S2, ndn = (size_t)R * KQ * KND;
    DevBuf dt;
    HIPCHK(dt.alloc(kbbq_tables_count(R, S2) * 8));
    HIPCHK(hipMemsetAsync(dt.p, 0, kbbq_tables_count(R, S2) * 8, c->stream));
    // K1 gives each of the R read groups its own walk over the rows and never meets a read of any other group: the reference's
    // IndexError for it (recalibrate.py:111-117 index the group axis) is found here, on every slab's sidecars as the slab is staged.
    // A read the kernels flag before it comes first; the read itself comes before anything else about it (the group is indexed first).
    int64_t stray = -1, bad = -1;
    // a slab: seq | cseq | qual | meta; when a read is flagged nothing reaches the caller's tables
    int rc = stage_run(c, "kbbq_accumulate", {seq, cseq, qual}, meta, nullptr, nreads, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kbbq_accumulate_dev(c, d, d + plane, d + 2 * plane, (const uint32_t*)(d + 3 * plane), m, pitch, R, S2, minscore, (int64_t*)dt.p);
    }, &bad, nullptr, [&](const uint32_t* w, int64_t lo, int64_t m) {
        if (stray >= 0 && stray < lo) return;
        for (int64_t i = 0; i < m; ++i) if ((int)((w[i] >> 16) & 0x7FFFu) >= R) { if (stray < 0 || lo + i < stray) stray = lo + i; return; }
    });
    if (rc && (stray < 0 || bad < 0 || bad < stray)) return rc;
    if (stray >= 0) return fail(KBBQ_E_INDEX, "read %lld: quality/read-group/cycle beyond the tables (reference: IndexError)", (long long)stray);
    std::vector<int64_t> h(kbbq_tables_count(R, S2));
    HIPCHK(hipMemcpyAsync(h.data(), dt.p, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < npos; ++i) { pos_errs[i] += h[i]; pos_total[i] += h[npos + i]; }
    for (size_t i = 0; i < ndn; ++i) { dinuc_errs[i] += h[2 * npos + i]; dinuc_total[i] += h[2 * npos + ndn + i]; }
    return KBBQ_OK;
}

int kbbq_apply(kbbq_ctx* c, const uint8_t* seq, const uint8_t* qual, const uint32_t* meta,
               int64_t nreads, int pitch, int R, int Qt, int S2, int D, int minscore,
               const int64_t* meanq, const int64_t* rgdq, const int64_t* qdq,
               const int64_t* posdq, const int64_t* dinucdq, uint8_t* qual_out)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nreads < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "kbbq_apply: bad nreads/pitch");
    if (nreads > 0 && (!seq || !qual || !meta || !qual_out)) return fail(KBBQ_E_ARG, "kbbq_apply: NULL plane");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> lut((kbbq_lut_bytes(R, Qt, S2) + 7) / 8);      // 8-byte words: aligned storage
    int flags = 0;
    int rc = kbbq_build_lut(R, Qt, S2, D, minscore, meanq, rgdq, qdq, posdq, dinucdq, lut.data(), &flags);
    if (rc) return rc;
    DevBuf dl;
    HIPCHK(dl.alloc(lut.size() * 8));
    HIPCHK(hipMemcpyAsync(dl.p, lut.data(), lut.size() * 8, hipMemcpyHostToDevice, c->stream));
    int mode = flags ? KBBQ_APPLY_CHECKED : KBBQ_APPLY_FAST;
    // a slab: seq | qual | out | meta (the output plane travels back from the same device slab).  Rows the fast kernel of one read
    // group only reports (kbbq_apply_dev) run again in checked mode: the caller sees their output or the reference's error, never KBBQ_E_LUT
    return stage_run(c, "kbbq_apply", {seq, qual}, meta, qual_out, nreads, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kbbq_apply_dev(c, d, d + plane, (const uint32_t*)(d + 3 * plane), m, pitch, R, Qt, S2, minscore, dl.p, mode, d + 2 * plane);
    }, nullptr, [&]() { const bool was_fast = mode == KBBQ_APPLY_FAST; mode = KBBQ_APPLY_CHECKED; return was_fast; });
}

// ---- ApplyBQSR on aligned rows (kbbq_apply_aligned.h) -----------------------------------------------------------------------
// d_qmap: the 256-byte map of kbbq_apply_aligned_q_dev, or NULL -- then the launch is kbbq_apply_aligned_dev's, kernel and bytes
static int apply_aligned_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint8_t* d_oq, const uint32_t* d_meta,
                             int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* d_model, int mode, uint8_t* d_out,
                             const uint8_t* d_qmap)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (!d_qual) d_qual = d_oq;
    if (!d_oq) d_oq = d_qual;
    int rc = check_planes("kbbq_apply_aligned_dev", n, pitch, d_seq, d_qual, d_out);
    if (rc) return rc;
    if ((uintptr_t)d_oq & 15) return fail(KBBQ_E_ARG, "kbbq_apply_aligned_dev: planes must be 16-byte aligned");
    if (n > 0 && (!d_seq || !d_qual || !d_meta || !d_out || !d_model)) return fail(KBBQ_E_ARG, "kbbq_apply_aligned_dev: NULL argument");
    if (mode != KBBQ_ALIGNED_LUT && mode != KBBQ_ALIGNED_F64) return fail(KBBQ_E_ARG, "kbbq_apply_aligned_dev: bad mode %d", mode);
    if (R <= 0 || R > 4096 || Qt <= 0 || Qt > (mode == KBBQ_ALIGNED_LUT ? 95 : 223) || S2 <= 0 || S2 > 65536)
        return fail(KBBQ_E_ARG, "kbbq_apply_aligned_dev: bad table shape R=%d Qt=%d S2=%d (R <= 4096)", R, Qt, S2);
    if (minscore < 0 || minscore > 222) return fail(KBBQ_E_ARG, "kbbq_apply_aligned_dev: minscore out of range");
    if ((uintptr_t)d_model & 15) return fail(KBBQ_E_ARG, "kbbq_apply_aligned_dev: the model must be 16-byte aligned");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    AaParams p;
    p.cpr = pitch / 16; p.pitch = pitch; p.Qt = Qt; p.S2 = S2; p.minscore = minscore;
    p.lut = reinterpret_cast<const int16_t*>(d_model); p.rs = lut_row_stride(S2);
    p.f64 = reinterpret_cast<const double*>(d_model); p.rs64 = AA_F64_FIXED + S2;
    p.status = c->d_status; p.qmap = d_qmap;
    // launches of at most 2^31 chunks (32-bit chunk numbers in the kernel)
    const int64_t per = std::max<int64_t>(1, ((int64_t)1 << 31) / p.cpr);
    for (int64_t lo = 0; lo < n; lo += per) {
        const int64_t m = std::min(per, n - lo);
        const size_t off = (size_t)lo * pitch;
        p.seq = d_seq + off; p.qual = d_qual + off; p.oq = d_oq + off; p.meta = d_meta + lo; p.out = d_out + off;
        p.nchunks = (u32)(m * p.cpr); p.row0 = lo;
        const unsigned grid = (unsigned)(((int64_t)p.nchunks + AA_THREADS - 1) / AA_THREADS);
        {
            Timed t(c, 1);
            if (d_qmap) {
                if (mode == KBBQ_ALIGNED_LUT) hipLaunchKernelGGL((kaa_apply<AA_LUT, true>), dim3(grid), dim3(AA_THREADS), 0, c->stream, p);
                else hipLaunchKernelGGL((kaa_apply<AA_F64, true>), dim3(grid), dim3(AA_THREADS), 0, c->stream, p);
            }
            else if (mode == KBBQ_ALIGNED_LUT) hipLaunchKernelGGL(kaa_apply<AA_LUT>, dim3(grid), dim3(AA_THREADS), 0, c->stream, p);
            else hipLaunchKernelGGL(kaa_apply<AA_F64>, dim3(grid), dim3(AA_THREADS), 0, c->stream, p);
        }
        HIPCHK(hipGetLastError());
    }
    return KBBQ_OK;
}

int kbbq_apply_aligned_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint8_t* d_oq, const uint32_t* d_meta,
                           int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* d_model, int mode, uint8_t* d_out)
{
    return apply_aligned_dev(c, d_seq, d_qual, d_oq, d_meta, n, pitch, R, Qt, S2, minscore, d_model, mode, d_out, nullptr);
}

int kbbq_apply_aligned_q_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint8_t* d_oq, const uint32_t* d_meta,
                             int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* d_model, int mode, uint8_t* d_out,
                             const uint8_t* d_qmap)
{
    return apply_aligned_dev(c, d_seq, d_qual, d_oq, d_meta, n, pitch, R, Qt, S2, minscore, d_model, mode, d_out, d_qmap);
}

// ---- static quantized qualities on a byte plane (kbbq_quantize_kernels.h) ----------------------------------------------------
int kbbq_quantize_plane_dev(kbbq_ctx* c, uint8_t* d_plane, int64_t nbytes, const uint8_t* d_qmap)
{
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (nbytes < 0 || (nbytes & 15)) return fail(KBBQ_E_ARG, "kbbq_quantize_plane_dev: nbytes must be a multiple of 16, got %lld", (long long)nbytes);
    if ((uintptr_t)d_plane & 15) return fail(KBBQ_E_ARG, "kbbq_quantize_plane_dev: the plane must be 16-byte aligned");
    if (nbytes == 0) return KBBQ_OK;
    if (!d_plane || !d_qmap) return fail(KBBQ_E_ARG, "kbbq_quantize_plane_dev: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    const long long nchunks = nbytes / 16;
    const long long per_wg = (long long)KQ_THREADS * KQ_CHUNKS_PER_LANE;
    const unsigned grid = (unsigned)std::min<long long>((nchunks + per_wg - 1) / per_wg, 1 << 16);
    hipLaunchKernelGGL(kq_plane, dim3(grid), dim3(KQ_THREADS), 0, c->stream, d_plane, nchunks, d_qmap);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

int kbbq_apply_aligned(kbbq_ctx* c, const uint8_t* seq, const uint8_t* qual, const uint8_t* oq, const uint32_t* meta,
                       int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* model, size_t model_bytes,
                       int mode, uint8_t* out, int64_t* bad_read)
{
    return kbbq_apply_aligned_q(c, seq, qual, oq, meta, n, pitch, R, Qt, S2, minscore, model, model_bytes, mode, out, bad_read, nullptr);
}

int kbbq_apply_aligned_q(kbbq_ctx* c, const uint8_t* seq, const uint8_t* qual, const uint8_t* oq, const uint32_t* meta,
                         int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* model, size_t model_bytes,
                         int mode, uint8_t* out, int64_t* bad_read, const uint8_t* qmap)
{
    if (bad_read) *bad_read = -1;
    if (!c) return fail(KBBQ_E_ARG, "ctx is NULL");
    if (n < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "kbbq_apply_aligned: bad n/pitch");
    if (!qual) qual = oq;
    if (!oq) oq = qual;
    if (n > 0 && (!seq || !qual || !meta || !out)) return fail(KBBQ_E_ARG, "kbbq_apply_aligned: NULL plane");
    if (!model || !model_bytes) return fail(KBBQ_E_ARG, "kbbq_apply_aligned: no model");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    DevBuf dm;
    // the model, and behind it (16-byte aligned) the 256-byte map where there is one: one allocation, uploaded once
    const size_t map_at = (model_bytes + 15) & ~(size_t)15;
    HIPCHK(dm.alloc(map_at + (qmap ? 256 : 0)));
    HIPCHK(hipMemcpyAsync(dm.p, model, model_bytes, hipMemcpyHostToDevice, c->stream));
    const uint8_t* d_qmap = nullptr;
    if (qmap) {
        d_qmap = (const uint8_t*)dm.p + map_at;
        HIPCHK(hipMemcpyAsync((void*)d_qmap, qmap, 256, hipMemcpyHostToDevice, c->stream));
    }
    // a slab: seq | qual | (oq) | out | meta (one quality plane when both are the same array)
    const int nq = qual == oq ? 1 : 2;
    auto launch = [&](uint8_t* d, size_t plane, int64_t m) {
        return apply_aligned_dev(c, d, d + plane, d + nq * plane, (const uint32_t*)(d + (nq + 2) * plane), m, pitch,
                                 R, Qt, S2, minscore, dm.p, mode, d + (nq + 1) * plane, d_qmap);
    };
    const char* who = qmap ? "kbbq_apply_aligned_q" : "kbbq_apply_aligned";
    if (nq == 1) return stage_run(c, who, {seq, qual}, meta, out, n, pitch, launch, bad_read);
    return stage_run(c, who, {seq, qual, oq}, meta, out, n, pitch, launch, bad_read);
}

// ---- k-mer counting and correction (kbbq_kmer.h) ------------------------------------------------------------------------------
struct kbbq_kmer_table {
    int k = 0;
    int64_t slots = 0;
    u64* keys = nullptr;              // [slots], KM_EMPTY where free
    u32* counts = nullptr;            // [slots]
};

size_t kbbq_kmer_table_bytes(int64_t slots) { return slots > 0 ? (size_t)slots * 12 : 0; }

int kbbq_kmer_table_create_dev(kbbq_ctx* c, int k, int64_t slots, kbbq_kmer_table** out)
{
    if (!c || !out) return fail(KBBQ_E_ARG, "kbbq_kmer_table_create_dev: NULL argument");
    *out = nullptr;
    if (k < 8 || k > 32) return fail(KBBQ_E_ARG, "kbbq_kmer_table_create_dev: k must be in 8..32, got %d", k);
    if (slots < 16 || (slots & (slots - 1)) || slots > ((int64_t)1 << 40))
        return fail(KBBQ_E_ARG, "kbbq_kmer_table_create_dev: slots must be a power of two in 16..2^40, got %lld", (long long)slots);
    HIPCHK(hipSetDevice(c->device));
    kbbq_kmer_table* t = new kbbq_kmer_table;
    t->k = k; t->slots = slots;
    hipError_t e = hipMalloc((void**)&t->keys, (size_t)slots * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&t->counts, (size_t)slots * 4);
    if (e == hipSuccess) e = hipMemsetAsync(t->keys, 0xFF, (size_t)slots * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->counts, 0, (size_t)slots * 4, c->stream);
    if (e != hipSuccess) {
        (void)kbbq_kmer_table_free_dev(c, t);
        return fail(KBBQ_E_HIP, "kbbq_kmer_table_create_dev: %lld slots (%zu bytes): %s", (long long)slots,
                    kbbq_kmer_table_bytes(slots), hipGetErrorString(e));
    }
    *out = t;
    return KBBQ_OK;
}

int kbbq_kmer_table_free_dev(kbbq_ctx* c, kbbq_kmer_table* t)
{
    if (!t) return KBBQ_OK;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
    if (t->keys) (void)hipFree(t->keys);
    if (t->counts) (void)hipFree(t->counts);
    delete t;
    return KBBQ_OK;
}

int kbbq_kmer_table_info(const kbbq_kmer_table* t, int* k, int64_t* slots, void** d_keys, void** d_counts)
{
    if (!t) return fail(KBBQ_E_ARG, "kbbq_kmer_table_info: table is NULL");
    if (k) *k = t->k;
    if (slots) *slots = t->slots;
    if (d_keys) *d_keys = t->keys;
    if (d_counts) *d_counts = t->counts;
    return KBBQ_OK;
}

// rows per workgroup and dynamic LDS of a kernel that walks k-mer windows and carves its LDS as `l`; the table's fields stay
// unset.  nib: 4-bit planes -- `pitch` bases a row in pitch / 2 bytes, rows 8-byte aligned.  passes: km_correct_passes', else 1
static int kmer_rows(kbbq_ctx* c, const char* who, int k, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                     bool nib, KmLds l, int passes, KmerParams& p, size_t* lds)
{
    int rc = check_planes(who, n, pitch, nib ? nullptr : d_seq, nullptr, nullptr);
    if (rc) return rc;
    if (nib && ((uintptr_t)d_seq & 7)) return fail(KBBQ_E_ARG, "%s: 4-bit planes must be 8-byte aligned", who);
    if (n > 0 && (!d_seq || !d_meta)) return fail(KBBQ_E_ARG, "%s: NULL plane or meta", who);
    p.seq = d_seq; p.meta = d_meta; p.nrows = n; p.pitch = nib ? pitch / 2 : pitch; p.cpr = pitch / 16; p.k = k;
    p.rows_per_wg = std::max(1, KM_THREADS / p.cpr);
    p.keys = nullptr; p.counts = nullptr; p.mask = 0; p.status = c->d_status;
    p.min_count = 1; p.out = nullptr; p.changed = nullptr; p.unresolved = nullptr;
    *lds = km_lds_bytes(l, p.rows_per_wg, p.cpr);
    if (*lds <= (size_t)c->lds_bytes) return KBBQ_OK;
    if (passes > 1)
        return fail(KBBQ_E_ARG, "%s: pitch %d needs %zu bytes of LDS with passes = %d (> %d)", who, pitch, *lds, passes, c->lds_bytes);
    return fail(KBBQ_E_ARG, "%s: pitch %d needs %zu bytes of LDS", who, pitch, *lds);
}

// ... of the count / correct kernels
static int kmer_geometry(kbbq_ctx* c, const char* who, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta,
                         int64_t n, int pitch, bool nib, KmLds l, int passes, KmerParams& p, size_t* lds)
{
    if (!c || !t) return fail(KBBQ_E_ARG, "%s: NULL ctx or table", who);
    int rc = kmer_rows(c, who, t->k, d_seq, d_meta, n, pitch, nib, l, passes, p, lds);
    if (rc) return rc;
    p.keys = t->keys; p.counts = t->counts; p.mask = (u64)t->slots - 1;
    return KBBQ_OK;
}

// the instantiation of a window kernel for the rows' reader
#define KM_READER(K, nib) ((nib) ? (const void*)K<true> : (const void*)K<false>)

// launches of at most 2^20 workgroups.  The kernel's parameters after its KmerParams, in their order: `extra` (KmerFilterParams,
// passes, KmerPartParams) when the kernel has one, `part` (the KmerPartParams of a kernel that has an `extra` before it), then
// `tally` -- both correction kernels end in a KmerTally, a copy of which moves with the rows of each launch; every other kernel
// gets nullptr.  `gate`: km_gate's one parameter after its KmerParams, whose quality and output planes move with the rows too
static int kmer_launches(kbbq_ctx* c, const KmerParams& p, const void* kernel, size_t lds, const void* extra,
                         const KmerTally* tally = nullptr, const KmerPartParams* part = nullptr, const KmerGate* gate = nullptr)
{
    HIPCHK(hipSetDevice(c->device));
    const int64_t per = ((int64_t)1 << 20) * p.rows_per_wg;
    for (int64_t lo = 0; lo < p.nrows; lo += per) {
        KmerParams q = p;
        const int64_t m = std::min(per, p.nrows - lo);
        q.seq = p.seq + (size_t)lo * p.pitch; q.meta = p.meta + lo; q.nrows = m;
        if (p.out) q.out = p.out + (size_t)lo * p.pitch;
        if (p.changed) q.changed = p.changed + lo;
        if (p.unresolved) q.unresolved = p.unresolved + lo;
        KmerTally ty = {nullptr, nullptr};
        if (tally && tally->qual) ty = {tally->qual + (size_t)lo * p.cpr * 16, tally->out + (size_t)lo * p.cpr * 16};
        void* args[4] = {&q, nullptr, nullptr, nullptr};   // hipLaunchKernel reads one entry per kernel parameter
        int na = 1;
        if (extra) args[na++] = const_cast<void*>(extra);
        if (part) args[na++] = const_cast<KmerPartParams*>(part);
        if (tally) args[na++] = &ty;
        KmerGate g = {nullptr, 0, nullptr, nullptr};
        if (gate) {
            g = *gate;
            g.qual = gate->qual + (size_t)lo * p.cpr * 16; g.out = gate->out + (size_t)lo * p.pitch;
            args[na++] = &g;
        }
        HIPCHK(hipLaunchKernel(kernel, dim3((unsigned)((m + p.rows_per_wg - 1) / p.rows_per_wg)), dim3(KM_THREADS), args, lds, c->stream));
    }
    return KBBQ_OK;
}

// the partition of a kbbq_kmer_count*_part* call, refused on the two numbers alone
static int kmer_part_ok(const char* who, int parts, int part)
{
    if (parts < 1 || parts > KM_MAX_BUCKETS) return fail(KBBQ_E_ARG, "%s: parts must be in 1..%d, got %d", who, KM_MAX_BUCKETS, parts);
    if (part < 0 || part >= parts) return fail(KBBQ_E_ARG, "%s: part must be in 0..%d (parts - 1), got %d", who, parts - 1, part);
    return KBBQ_OK;
}

// parts == 1: km_count itself; else the windows of partition `part` of `parts` (km_count_part)
static int kmer_count_rows(kbbq_ctx* c, const char* who, kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n,
                           int pitch, bool nib, int parts = 1, int part = 0)
{
    int rc = kmer_part_ok(who, parts, part);
    if (rc) return rc;
    KmerParams p; size_t lds = 0;
    rc = kmer_geometry(c, who, t, d_seq, d_meta, n, pitch, nib, KM_LDS_COUNT, 1, p, &lds);
    if (rc || n == 0) return rc;
    if (parts == 1) return kmer_launches(c, p, KM_READER(km_count, nib), lds, nullptr);
    const KmerPartParams pp = {(u32)parts, (u32)part};
    return kmer_launches(c, p, KM_READER(km_count_part, nib), lds, &pp);
}

int kbbq_kmer_count_dev(kbbq_ctx* c, kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch)
{
    return kmer_count_rows(c, "kbbq_kmer_count_dev", t, d_seq, d_meta, n, pitch, false);
}

// the KBBQ_ROWS_* flags of the k-mer calls on resident rows: is the plane a 4-bit one?  Two reads to a row need nothing of
// their own (the separator is a break); their pitch holds at least 2 x 1 bases and the separator, as any multiple of 16 does
static int kmer_row_flags(const char* who, int flags, bool* nib)
{
    int rc = layout_flags_ok(who, flags);
    if (rc) return rc;
    *nib = (flags & KBBQ_ROWS_NIBBLES) != 0;
    return KBBQ_OK;
}

int kbbq_kmer_count_rows_dev(kbbq_ctx* c, kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows, int pitch,
                             int flags)
{
    bool nib = false;
    int rc = kmer_row_flags("kbbq_kmer_count_rows_dev", flags, &nib);
    if (rc) return rc;
    return kmer_count_rows(c, "kbbq_kmer_count_rows_dev", t, d_seq, d_meta, nrows, pitch, nib);
}

int kbbq_kmer_count_part_dev(kbbq_ctx* c, kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                             int parts, int part)
{
    return kmer_count_rows(c, "kbbq_kmer_count_part_dev", t, d_seq, d_meta, n, pitch, false, parts, part);
}

int kbbq_kmer_count_rows_part_dev(kbbq_ctx* c, kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                                  int pitch, int flags, int parts, int part)
{
    bool nib = false;
    int rc = kmer_part_ok("kbbq_kmer_count_rows_part_dev", parts, part);
    if (!rc) rc = kmer_row_flags("kbbq_kmer_count_rows_part_dev", flags, &nib);
    if (rc) return rc;
    return kmer_count_rows(c, "kbbq_kmer_count_rows_part_dev", t, d_seq, d_meta, nrows, pitch, nib, parts, part);
}

int kbbq_kmer_histogram_dev(kbbq_ctx* c, const kbbq_kmer_table* t, uint64_t* d_hist)
{
    if (!c || !t || !d_hist) return fail(KBBQ_E_ARG, "kbbq_kmer_histogram_dev: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(d_hist, 0, KM_HIST * 8, c->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((t->slots + KM_THREADS - 1) / KM_THREADS, (int64_t)c->cus * 8);
    hipLaunchKernelGGL(km_histogram, dim3(grid), dim3(KM_THREADS), 0, c->stream, t->keys, t->counts, (u64)t->slots,
                       reinterpret_cast<u64*>(d_hist));
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// Which of the correction kernels a call wants.  passes: 1 km_correct, 2..KM_MAX_PASSES km_correct_passes.
// pairs (KBBQ_ROWS_PAIRS) matter to the N rule alone: the separator of two reads is no N.
// tally: the corrected form that also writes the tally plane (kbbq_kmer_correct_rows_skip_dev)
struct KmerForm { bool nib; int fixn; bool flags, unres; int passes; bool tally = false; };

static KmerForm kmer_form_rows(bool nib, bool pairs, int opts, int passes)
{
    return {nib, !(opts & KBBQ_KMER_FIX_N) ? KM_FIXN_OFF : pairs ? KM_FIXN_PAIRS : KM_FIXN_READS, false, false, passes};
}

// ... and the kernel of a form: [several passes][reader x KM_FIXN_*, the flag form, the flag form with unresolved bases,
// reader x KM_FIXN_* with the tally plane]
#define KM_FORMS(K) {(const void*)K<false, KM_FIXN_OFF>, (const void*)K<false, KM_FIXN_READS>, (const void*)K<false, KM_FIXN_PAIRS>, \
                     (const void*)K<true, KM_FIXN_OFF>, (const void*)K<true, KM_FIXN_READS>, (const void*)K<true, KM_FIXN_PAIRS>,    \
                     (const void*)K<false, KM_FIXN_OFF, true>, (const void*)K<false, KM_FIXN_OFF, true, true>,                       \
                     (const void*)K<false, KM_FIXN_OFF, false, false, true>, (const void*)K<false, KM_FIXN_READS, false, false, true>, \
                     (const void*)K<false, KM_FIXN_PAIRS, false, false, true>, (const void*)K<true, KM_FIXN_OFF, false, false, true>,  \
                     (const void*)K<true, KM_FIXN_READS, false, false, true>, (const void*)K<true, KM_FIXN_PAIRS, false, false, true>}
static const void* const KM_CORRECT[2][14] = {KM_FORMS(km_correct), KM_FORMS(km_correct_passes)};

static const void* kmer_correct_kernel(const KmerForm& f, KmLds* l)
{
    *l = f.passes > 1 ? KM_LDS_PASSES : KM_LDS_CORRECT;
    return KM_CORRECT[f.passes > 1][f.flags ? 6 + (f.unres ? 1 : 0) : (f.tally ? 8 : 0) + (f.nib ? 3 : 0) + f.fixn];
}

// the `opts` word of the kbbq_kmer_correct*_ex calls (not the KBBQ_ROWS_* flags): checked before anything is launched
static int kmer_correct_opts(const char* who, int opts)
{
    if (opts & ~KBBQ_KMER_FIX_N) return fail(KBBQ_E_ARG, "%s: unknown bits in opts 0x%x (KBBQ_KMER_FIX_N = %d)", who, opts, KBBQ_KMER_FIX_N);
    return KBBQ_OK;
}

// the `passes` of the kbbq_kmer_*_passes* calls: checked before anything else
static int kmer_passes_ok(const char* who, int passes)
{
    if (passes < 1 || passes > KM_MAX_PASSES) return fail(KBBQ_E_ARG, "%s: passes must be in 1..%d, got %d", who, KM_MAX_PASSES, passes);
    return KBBQ_OK;
}

// d_out: the corrected plane, with f.flags the flag plane; d_unresolved (may be NULL): the per-row count of 2s of the flag form
// or of the zeros f.tally writes, zeroed here when the form writes none.  ty: f.tally's planes, checked by the caller.
// The caller has checked its opts and passes.
static int kmer_correct_rows(kbbq_ctx* c, const char* who, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta,
                             int64_t n, int pitch, int min_count, uint8_t* d_out, uint32_t* d_changed, uint32_t* d_unresolved,
                             const KmerForm& f, KmerTally ty = {nullptr, nullptr})
{
    KmerParams p; size_t lds = 0; KmLds l;
    const void* kernel = kmer_correct_kernel(f, &l);
    int rc = kmer_geometry(c, who, t, d_seq, d_meta, n, pitch, f.nib, l, f.passes, p, &lds);
    if (rc) return rc;
    if (min_count < 1) return fail(KBBQ_E_ARG, "%s: min_count must be >= 1, got %d", who, min_count);
    if (n > 0 && (!d_out || ((uintptr_t)d_out & (f.nib ? 7 : 15))))
        return fail(KBBQ_E_ARG, "%s: d_out NULL or not %d-byte aligned", who, f.nib ? 8 : 16);
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));                    // for the memset and the attribute; kmer_launches sets it for the other paths
    p.min_count = (u32)min_count; p.out = d_out; p.changed = d_changed;
    if (f.unres || f.tally) p.unresolved = d_unresolved;
    else if (d_unresolved) HIPCHK(hipMemsetAsync(d_unresolved, 0, (size_t)n * 4, c->stream));     // no byte is 2 without the option
    if (f.passes > 1 && lds > 64 * 1024)                // beyond what a kernel may take without asking
        HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, c->lds_bytes));
    // km_correct(KmerParams, KmerTally), km_correct_passes(KmerParams, int passes, KmerTally): this is their one launch site
    return kmer_launches(c, p, kernel, lds, f.passes > 1 ? &f.passes : nullptr, &ty);
}

// character rows, one read a row: opts and passes are checked here
static int kmer_correct_reads(kbbq_ctx* c, const char* who, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta,
                              int64_t n, int pitch, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts, int passes)
{
    int rc = kmer_passes_ok(who, passes);
    if (!rc) rc = kmer_correct_opts(who, opts);
    if (rc) return rc;
    return kmer_correct_rows(c, who, t, d_seq, d_meta, n, pitch, min_count, d_out, d_changed, nullptr, kmer_form_rows(false, false, opts, passes));
}

int kbbq_kmer_correct_ex_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                             int min_count, uint8_t* d_out, uint32_t* d_changed, int opts)
{
    return kmer_correct_reads(c, "kbbq_kmer_correct_ex_dev", t, d_seq, d_meta, n, pitch, min_count, d_out, d_changed, opts, 1);
}

int kbbq_kmer_correct_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                          int min_count, uint8_t* d_out, uint32_t* d_changed)
{
    return kmer_correct_reads(c, "kbbq_kmer_correct_dev", t, d_seq, d_meta, n, pitch, min_count, d_out, d_changed, 0, 1);
}

int kbbq_kmer_correct_passes_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                                 int min_count, uint8_t* d_out, uint32_t* d_changed, int opts, int passes)
{
    return kmer_correct_reads(c, "kbbq_kmer_correct_passes_dev", t, d_seq, d_meta, n, pitch, min_count, d_out, d_changed, opts, passes);
}

// the flag form.  Its opts are its own: 0 or KBBQ_KMER_FLAG_UNRESOLVED
static int kmer_flag_rows(kbbq_ctx* c, const char* who, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n,
                          int pitch, int min_count, uint8_t* d_flags, uint32_t* d_changed, uint32_t* d_unresolved, int opts, int passes)
{
    int rc = kmer_passes_ok(who, passes);
    if (rc) return rc;
    if (opts & ~KBBQ_KMER_FLAG_UNRESOLVED)
        return fail(KBBQ_E_ARG, "%s: opts 0x%x: the flag form takes KBBQ_KMER_FLAG_UNRESOLVED (%d) alone%s", who, opts,
                    KBBQ_KMER_FLAG_UNRESOLVED, (opts & KBBQ_KMER_FIX_N) ? " (it has no N rule)" : "");
    // kbbq_kmer_correct_dev's refusals; those of the numbers alone come first, so that they need no context to be decided
    rc = check_planes(who, n, pitch, d_seq, d_flags, nullptr);
    if (rc) return rc;
    if (min_count < 1) return fail(KBBQ_E_ARG, "%s: min_count must be >= 1, got %d", who, min_count);
    return kmer_correct_rows(c, who, t, d_seq, d_meta, n, pitch, min_count, d_flags, d_changed, d_unresolved,
                             {false, KM_FIXN_OFF, true, (opts & KBBQ_KMER_FLAG_UNRESOLVED) != 0, passes});
}

int kbbq_kmer_flag_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                       int min_count, uint8_t* d_flags, uint32_t* d_changed)
{
    return kmer_flag_rows(c, "kbbq_kmer_flag_dev", t, d_seq, d_meta, n, pitch, min_count, d_flags, d_changed, nullptr, 0, 1);
}

int kbbq_kmer_flag_ex_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                          int min_count, uint8_t* d_flags, uint32_t* d_changed, uint32_t* d_unresolved, int opts)
{
    return kmer_flag_rows(c, "kbbq_kmer_flag_ex_dev", t, d_seq, d_meta, n, pitch, min_count, d_flags, d_changed, d_unresolved, opts, 1);
}

int kbbq_kmer_flag_passes_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch,
                              int min_count, uint8_t* d_flags, uint32_t* d_changed, uint32_t* d_unresolved, int opts, int passes)
{
    return kmer_flag_rows(c, "kbbq_kmer_flag_passes_dev", t, d_seq, d_meta, n, pitch, min_count, d_flags, d_changed, d_unresolved, opts, passes);
}

// resident rows of either reader, one or two reads a row (KBBQ_ROWS_*)
static int kmer_correct_rows_flags(kbbq_ctx* c, const char* who, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta,
                                   int64_t nrows, int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts,
                                   int passes)
{
    int rc = kmer_passes_ok(who, passes);
    if (!rc) rc = kmer_correct_opts(who, opts);
    bool nib = false;
    if (!rc) rc = kmer_row_flags(who, flags, &nib);
    if (rc) return rc;
    return kmer_correct_rows(c, who, t, d_seq, d_meta, nrows, pitch, min_count, d_out, d_changed, nullptr,
                             kmer_form_rows(nib, (flags & KBBQ_ROWS_PAIRS) != 0, opts, passes));
}

int kbbq_kmer_correct_rows_passes_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                                      int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts, int passes)
{
    return kmer_correct_rows_flags(c, "kbbq_kmer_correct_rows_passes_dev", t, d_seq, d_meta, nrows, pitch, flags, min_count, d_out, d_changed,
                                   opts, passes);
}

int kbbq_kmer_correct_rows_ex_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                                  int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts)
{
    return kmer_correct_rows_flags(c, "kbbq_kmer_correct_rows_ex_dev", t, d_seq, d_meta, nrows, pitch, flags, min_count, d_out, d_changed, opts, 1);
}

int kbbq_kmer_correct_rows_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                               int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed)
{
    return kmer_correct_rows_flags(c, "kbbq_kmer_correct_rows_dev", t, d_seq, d_meta, nrows, pitch, flags, min_count, d_out, d_changed, 0, 1);
}

// kbbq_kmer_correct_rows_passes_dev and the tally plane beside the corrected one
int kbbq_kmer_correct_rows_skip_dev(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                                    int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts, int passes,
                                    const uint8_t* d_qual, uint8_t* d_tally_qual, uint32_t* d_unresolved)
{
    const char* who = "kbbq_kmer_correct_rows_skip_dev";
    int rc = kmer_passes_ok(who, passes);
    if (!rc && (opts & KBBQ_KMER_FLAG_UNRESOLVED))
        rc = fail(KBBQ_E_ARG, "%s: opts 0x%x: KBBQ_KMER_FLAG_UNRESOLVED (%d) is the flag form's; here unresolved bases go to d_tally_qual",
                  who, opts, KBBQ_KMER_FLAG_UNRESOLVED);
    if (!rc) rc = kmer_correct_opts(who, opts);
    bool nib = false;
    if (!rc) rc = kmer_row_flags(who, flags, &nib);
    if (rc) return rc;
    if (!d_qual || !d_tally_qual) return fail(KBBQ_E_ARG, "%s: d_qual or d_tally_qual is NULL", who);
    if (d_tally_qual == d_qual) return fail(KBBQ_E_ARG, "%s: d_tally_qual is d_qual: the qualities as read must stay", who);
    if (((uintptr_t)d_qual | (uintptr_t)d_tally_qual) & 15) return fail(KBBQ_E_ARG, "%s: d_qual or d_tally_qual not 16-byte aligned", who);
    KmerForm f = kmer_form_rows(nib, (flags & KBBQ_ROWS_PAIRS) != 0, opts, passes);
    f.tally = true;
    return kmer_correct_rows(c, who, t, d_seq, d_meta, nrows, pitch, min_count, d_out, d_changed, d_unresolved, f, {d_qual, d_tally_qual});
}

// the quality gate in front of the count (csrc/kbbq_kmer.h km_gate): arguments checked, then kmer_launches
int kbbq_kmer_gate_rows_dev(kbbq_ctx* c, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows, int pitch,
                            int flags, int k, int qual_byte_min, uint8_t* d_out, uint64_t* d_windows)
{
    const char* who = "kbbq_kmer_gate_rows_dev";
    if (!c) return fail(KBBQ_E_ARG, "%s: NULL ctx", who);
    bool nib = false;
    int rc = kmer_row_flags(who, flags, &nib);
    if (rc) return rc;
    if (k < 8 || k > 32) return fail(KBBQ_E_ARG, "%s: k must be in 8..32, got %d", who, k);
    if (qual_byte_min < 1 || qual_byte_min > 255)
        return fail(KBBQ_E_ARG, "%s: qual_byte_min must be in 1..255, got %d", who, qual_byte_min);
    KmerParams p; size_t lds = 0;
    rc = kmer_rows(c, who, k, d_seq, d_meta, nrows, pitch, nib, KM_LDS_GATE, 1, p, &lds);
    if (rc) return rc;
    if (nrows > 0 && (!d_qual || !d_out)) return fail(KBBQ_E_ARG, "%s: NULL plane or meta", who);
    if (nrows > 0 && d_out == d_seq) return fail(KBBQ_E_ARG, "%s: d_out is d_seq: the rows as read must stay", who);
    if ((uintptr_t)d_qual & 15) return fail(KBBQ_E_ARG, "%s: d_qual not 16-byte aligned", who);
    if ((uintptr_t)d_out & (nib ? 7 : 15)) return fail(KBBQ_E_ARG, "%s: d_out not %d-byte aligned", who, nib ? 8 : 16);
    if ((uintptr_t)d_windows & 7) return fail(KBBQ_E_ARG, "%s: d_windows not 8-byte aligned", who);
    if (nrows == 0) return KBBQ_OK;
    const KmerGate g = {d_qual, (u32)qual_byte_min, d_out, reinterpret_cast<u64*>(d_windows)};
    return kmer_launches(c, p, KM_READER(km_gate, nib), lds, nullptr, nullptr, nullptr, &g);
}

int kbbq_kmer_table_clear_dev(kbbq_ctx* c, kbbq_kmer_table* t)
{
    if (!c || !t) return fail(KBBQ_E_ARG, "kbbq_kmer_table_clear_dev: NULL ctx or table");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(t->keys, 0xFF, (size_t)t->slots * 8, c->stream));
    HIPCHK(hipMemsetAsync(t->counts, 0, (size_t)t->slots * 4, c->stream));
    return KBBQ_OK;
}

uint32_t kbbq_kmer_owner(uint64_t key, int nbuckets) { return nbuckets > 0 ? km_owner(key, (u32)nbuckets) : 0u; }

static unsigned kmer_select_grid(const kbbq_ctx* c, const kbbq_kmer_table* t)
{
    const int64_t tiles = (t->slots / 4 + KM_THREADS * KM_SEL_QUADS - 1) / (KM_THREADS * KM_SEL_QUADS);
    return (unsigned)std::min<int64_t>(tiles, (int64_t)c->cus * 8);
}

int kbbq_kmer_select_sizes_dev(kbbq_ctx* c, const kbbq_kmer_table* t, int nbuckets, uint32_t min_count, int64_t* h_sizes)
{
    if (!c || !t || !h_sizes) return fail(KBBQ_E_ARG, "kbbq_kmer_select_sizes_dev: NULL argument");
    if (nbuckets < 1 || nbuckets > KM_MAX_BUCKETS)
        return fail(KBBQ_E_ARG, "kbbq_kmer_select_sizes_dev: nbuckets must be in 1..%d, got %d", KM_MAX_BUCKETS, nbuckets);
    HIPCHK(hipSetDevice(c->device));
    DevBuf d;
    HIPCHK(d.alloc((size_t)nbuckets * 8));
    HIPCHK(hipMemsetAsync(d.p, 0, (size_t)nbuckets * 8, c->stream));
    hipLaunchKernelGGL(km_select_sizes, dim3(kmer_select_grid(c, t)), dim3(KM_THREADS), 0, c->stream, t->keys, t->counts,
                       (u64)t->slots, min_count, (u32)nbuckets, (u64*)d.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_sizes, d.p, (size_t)nbuckets * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_kmer_select_dev(kbbq_ctx* c, const kbbq_kmer_table* t, int nbuckets, uint32_t min_count, const int64_t* h_offsets,
                         uint64_t* d_keys, uint32_t* d_counts)
{
    if (!c || !t || !h_offsets) return fail(KBBQ_E_ARG, "kbbq_kmer_select_dev: NULL argument");
    if (nbuckets < 1 || nbuckets > KM_MAX_BUCKETS)
        return fail(KBBQ_E_ARG, "kbbq_kmer_select_dev: nbuckets must be in 1..%d, got %d", KM_MAX_BUCKETS, nbuckets);
    for (int b = 0; b < nbuckets; ++b)
        if (h_offsets[b] < 0) return fail(KBBQ_E_ARG, "kbbq_kmer_select_dev: offset %d is negative", b);
    HIPCHK(hipSetDevice(c->device));
    std::vector<u64> cur((size_t)nbuckets * KM_CURSOR_STRIDE, 0);
    for (int b = 0; b < nbuckets; ++b) cur[(size_t)b * KM_CURSOR_STRIDE] = (u64)h_offsets[b];
    DevBuf d;
    HIPCHK(d.alloc(cur.size() * 8));
    HIPCHK(hipMemcpyAsync(d.p, cur.data(), cur.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(km_select_scatter, dim3(kmer_select_grid(c, t)), dim3(KM_THREADS), 0, c->stream, t->keys, t->counts,
                       (u64)t->slots, min_count, (u32)nbuckets, (u64*)d.p, (u64*)d_keys, (u32*)d_counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));          // the cursors (and the caller's offsets) are released on return
    return KBBQ_OK;
}

int kbbq_kmer_merge_dev(kbbq_ctx* c, kbbq_kmer_table* t, const uint64_t* d_keys, const uint32_t* d_counts, int64_t n)
{
    if (!c || !t) return fail(KBBQ_E_ARG, "kbbq_kmer_merge_dev: NULL ctx or table");
    if (n < 0 || (n > 0 && (!d_keys || !d_counts))) return fail(KBBQ_E_ARG, "kbbq_kmer_merge_dev: bad pairs");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    const unsigned grid = (unsigned)std::min<int64_t>((n + KM_THREADS - 1) / KM_THREADS, (int64_t)c->cus * 32);
    hipLaunchKernelGGL(km_merge, dim3(grid), dim3(KM_THREADS), 0, c->stream, (const u64*)d_keys, (const u32*)d_counts, n,
                       t->keys, t->counts, (u64)t->slots - 1, c->d_status);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

// ---- k-mer sets (kbbq_kmer_set.h; kbbq/kmerset.py) --------------------------------------------------------------------------
// The sort is rocPRIM's radix sort (header-only) over the 2k key bits: keys are unique, so the result is one permutation
// whatever the thread order.  Keys are sorted as the unsigned 64-bit words they are (k = 32 uses bit 63).
static hipError_t kmer_sort_pairs(void* temp, size_t& bytes, const u64* kin, u64* kout, const u32* cin, u32* cout, size_t n, int k,
                                  hipStream_t st)
{
    return rocprim::radix_sort_pairs(temp, bytes, kin, kout, cin, cout, n, 0u, (unsigned)(2 * k), st);
}

int kbbq_kmer_sort_pairs_bytes(kbbq_ctx* c, int64_t n, size_t* bytes)
{
    if (!c || !bytes) return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_bytes: NULL argument");
    if (n < 0) return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_bytes: n must be >= 0, got %lld", (long long)n);
    *bytes = 0;
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    size_t need = 0;
    HIPCHK(kmer_sort_pairs(nullptr, need, nullptr, nullptr, nullptr, nullptr, (size_t)n, 32, c->stream));
    *bytes = need;
    return KBBQ_OK;
}

int kbbq_kmer_sort_pairs_dev(kbbq_ctx* c, int k, const uint64_t* d_keys_in, const uint32_t* d_counts_in, uint64_t* d_keys_out,
                             uint32_t* d_counts_out, int64_t n, void* d_temp, size_t temp_bytes)
{
    if (!c) return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_dev: NULL ctx");
    if (k < 8 || k > 32) return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_dev: k must be in 8..32, got %d", k);
    if (n < 0) return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_dev: n must be >= 0, got %lld", (long long)n);
    if (n == 0) return KBBQ_OK;
    if (!d_keys_in || !d_counts_in || !d_keys_out || !d_counts_out) return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_dev: NULL pairs");
    if ((const void*)d_keys_in == (const void*)d_keys_out || (const void*)d_counts_in == (const void*)d_counts_out)
        return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_dev: the sorted pairs need buffers of their own");
    HIPCHK(hipSetDevice(c->device));
    size_t need = 0;
    HIPCHK(kmer_sort_pairs(nullptr, need, nullptr, nullptr, nullptr, nullptr, (size_t)n, 32, c->stream));
    if (need > 0 && (!d_temp || temp_bytes < need))
        return fail(KBBQ_E_ARG, "kbbq_kmer_sort_pairs_dev: the temporary holds %zu bytes, %zu are needed (kbbq_kmer_sort_pairs_bytes)",
                    d_temp ? temp_bytes : (size_t)0, need);
    HIPCHK(kmer_sort_pairs(d_temp, temp_bytes, (const u64*)d_keys_in, (u64*)d_keys_out, (const u32*)d_counts_in, (u32*)d_counts_out,
                           (size_t)n, k, c->stream));
    return KBBQ_OK;
}

int kbbq_kmer_check_pairs_dev(kbbq_ctx* c, const uint64_t* d_keys, const uint32_t* d_counts, int64_t n, int k, uint32_t keep,
                              int64_t first, int have_prev, uint64_t prev_key, uint64_t* h_sums, int64_t* bad_index, int* bad_reason)
{
    if (!c || !h_sums || !bad_index || !bad_reason) return fail(KBBQ_E_ARG, "kbbq_kmer_check_pairs_dev: NULL argument");
    if (k < 8 || k > 32) return fail(KBBQ_E_ARG, "kbbq_kmer_check_pairs_dev: k must be in 8..32, got %d", k);
    if (n < 0 || first < 0 || first > ((int64_t)1 << 60) - n)
        return fail(KBBQ_E_ARG, "kbbq_kmer_check_pairs_dev: bad n / first (%lld, %lld)", (long long)n, (long long)first);
    if (n > 0 && (!d_keys || !d_counts)) return fail(KBBQ_E_ARG, "kbbq_kmer_check_pairs_dev: NULL pairs");
    if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_counts & 3)) return fail(KBBQ_E_ARG, "kbbq_kmer_check_pairs_dev: pairs not aligned");
    *bad_index = -1; *bad_reason = 0;
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    DevBuf d;
    HIPCHK(d.alloc(3 * 8));
    u64 out[3] = {0, 0, KM_CHECK_NONE};
    HIPCHK(hipMemcpyAsync(d.p, out, sizeof out, hipMemcpyHostToDevice, c->stream));
    const KmerCheck q = {(const u64*)d_keys, (const u32*)d_counts, n, first, (u64)prev_key, have_prev ? 1u : 0u, k, keep, (u64*)d.p};
    const int64_t steps = (n + 1) / 2;
    const unsigned grid = (unsigned)std::min<int64_t>((steps + KM_THREADS - 1) / KM_THREADS, (int64_t)c->cus * 8);
    const bool vec = !((uintptr_t)d_keys & 15) && !((uintptr_t)d_counts & 7);
    if (vec) hipLaunchKernelGGL(km_check_pairs<true>, dim3(grid), dim3(KM_THREADS), 0, c->stream, q);
    else hipLaunchKernelGGL(km_check_pairs<false>, dim3(grid), dim3(KM_THREADS), 0, c->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d.p, sizeof out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    h_sums[0] += out[0]; h_sums[1] += out[1];
    if (out[2] != KM_CHECK_NONE) { *bad_index = (int64_t)(out[2] >> 3); *bad_reason = (int)(out[2] & 7); }
    return KBBQ_OK;
}

// kbbq_kmer_count and kbbq_kmer_count_part: `dev`, the device call a slab goes to, is named in a refusal that only it can make
static int kmer_count_host(kbbq_ctx* c, const char* who, const char* dev, kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta,
                           int64_t n, int pitch, int parts, int part)
{
    int rc = kmer_part_ok(who, parts, part);
    if (rc) return rc;
    if (!c || !t) return fail(KBBQ_E_ARG, "%s: NULL ctx or table", who);
    if (n < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "%s: bad n/pitch", who);
    if (n > 0 && (!seq || !meta)) return fail(KBBQ_E_ARG, "%s: NULL plane", who);
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    // a slab: seq | meta
    return stage_run(c, who, {seq}, meta, nullptr, n, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kmer_count_rows(c, dev, t, d, (const uint32_t*)(d + plane), m, pitch, false, parts, part);
    });
}

int kbbq_kmer_count(kbbq_ctx* c, kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch)
{
    return kmer_count_host(c, "kbbq_kmer_count", "kbbq_kmer_count_dev", t, seq, meta, n, pitch, 1, 0);
}

int kbbq_kmer_count_part(kbbq_ctx* c, kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch, int parts,
                         int part)
{
    return kmer_count_host(c, "kbbq_kmer_count_part", "kbbq_kmer_count_part_dev", t, seq, meta, n, pitch, parts, part);
}

static int kmer_correct_host(kbbq_ctx* c, const char* who, const kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta, int64_t n,
                             int pitch, int min_count, uint8_t* out, uint32_t* changed, int opts, int passes)
{
    int orc = kmer_passes_ok(who, passes);
    if (!orc) orc = kmer_correct_opts(who, opts);
    if (orc) return orc;
    if (!c || !t) return fail(KBBQ_E_ARG, "%s: NULL ctx or table", who);
    if (n < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "%s: bad n/pitch", who);
    if (n > 0 && (!seq || !meta || !out)) return fail(KBBQ_E_ARG, "%s: NULL plane", who);
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    DevBuf dc;
    if (changed) HIPCHK(dc.alloc((size_t)n * 4));
    // a slab: seq | out | meta; the slabs run in order, `done` rows before this one
    int64_t done = 0;
    int rc = stage_run(c, who, {seq}, meta, out, n, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        if (done + m > n) return fail(KBBQ_E_HIP, "%s: more rows launched than given", who);
        uint32_t* dch = changed ? (uint32_t*)dc.p + done : nullptr;
        done += m;
        return kmer_correct_rows(c, who, t, d, (const uint32_t*)(d + 2 * plane), m, pitch, min_count, d + plane, dch, nullptr,
                                 kmer_form_rows(false, false, opts, passes));
    });
    if (rc || !changed) return rc;
    HIPCHK(hipMemcpyAsync(changed, dc.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_kmer_correct_ex(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch,
                         int min_count, uint8_t* out, uint32_t* changed, int opts)
{
    return kmer_correct_host(c, "kbbq_kmer_correct_ex", t, seq, meta, n, pitch, min_count, out, changed, opts, 1);
}

int kbbq_kmer_correct_passes(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch,
                             int min_count, uint8_t* out, uint32_t* changed, int opts, int passes)
{
    return kmer_correct_host(c, "kbbq_kmer_correct_passes", t, seq, meta, n, pitch, min_count, out, changed, opts, passes);
}

int kbbq_kmer_correct(kbbq_ctx* c, const kbbq_kmer_table* t, const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch,
                      int min_count, uint8_t* out, uint32_t* changed)
{
    return kmer_correct_host(c, "kbbq_kmer_correct", t, seq, meta, n, pitch, min_count, out, changed, 0, 1);
}

// ---- prefilter: k-mers seen once stay out of the table (kbbq_kmer.h) ----------------------------------------------------------
struct kbbq_kmer_filter {
    int64_t words = 0;
    u64* seen = nullptr;              // [words]; NULL after kbbq_kmer_filter_release_seen_dev
    u64* twice = nullptr;             // [words]
    u64* admitted = nullptr;          // one counter
};

size_t kbbq_kmer_filter_bytes(int64_t words) { return words > 0 ? (size_t)words * 16 : 0; }

int kbbq_kmer_filter_create_dev(kbbq_ctx* c, int64_t words, kbbq_kmer_filter** out)
{
    if (!c || !out) return fail(KBBQ_E_ARG, "kbbq_kmer_filter_create_dev: NULL argument");
    *out = nullptr;
    if (words < 1 || (words & (words - 1)) || words > ((int64_t)1 << 40))
        return fail(KBBQ_E_ARG, "kbbq_kmer_filter_create_dev: words must be a power of two in 1..2^40, got %lld", (long long)words);
    HIPCHK(hipSetDevice(c->device));
    kbbq_kmer_filter* f = new kbbq_kmer_filter;
    f->words = words;
    hipError_t e = hipMalloc((void**)&f->seen, (size_t)words * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&f->twice, (size_t)words * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&f->admitted, 8);
    if (e == hipSuccess) e = hipMemsetAsync(f->seen, 0, (size_t)words * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(f->twice, 0, (size_t)words * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(f->admitted, 0, 8, c->stream);
    if (e != hipSuccess) {
        (void)kbbq_kmer_filter_free_dev(c, f);
        return fail(KBBQ_E_HIP, "kbbq_kmer_filter_create_dev: %lld words (%zu bytes): %s", (long long)words,
                    kbbq_kmer_filter_bytes(words), hipGetErrorString(e));
    }
    *out = f;
    return KBBQ_OK;
}

int kbbq_kmer_filter_free_dev(kbbq_ctx* c, kbbq_kmer_filter* f)
{
    if (!f) return KBBQ_OK;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
    if (f->seen) (void)hipFree(f->seen);
    if (f->twice) (void)hipFree(f->twice);
    if (f->admitted) (void)hipFree(f->admitted);
    delete f;
    return KBBQ_OK;
}

int kbbq_kmer_filter_release_seen_dev(kbbq_ctx* c, kbbq_kmer_filter* f)
{
    if (!c || !f) return fail(KBBQ_E_ARG, "kbbq_kmer_filter_release_seen_dev: NULL ctx or filter");
    if (!f->seen) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));            // the last prefilter pass has run
    HIPCHK(hipFree(f->seen));
    f->seen = nullptr;
    return KBBQ_OK;
}

int kbbq_kmer_filter_clear_dev(kbbq_ctx* c, kbbq_kmer_filter* f)
{
    if (!c || !f) return fail(KBBQ_E_ARG, "kbbq_kmer_filter_clear_dev: NULL ctx or filter");
    if (!f->seen) return fail(KBBQ_E_ARG, "kbbq_kmer_filter_clear_dev: the filter's `seen` array has been released");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(f->seen, 0, (size_t)f->words * 8, c->stream));
    HIPCHK(hipMemsetAsync(f->twice, 0, (size_t)f->words * 8, c->stream));
    HIPCHK(hipMemsetAsync(f->admitted, 0, 8, c->stream));
    return KBBQ_OK;
}

int kbbq_kmer_filter_info(const kbbq_kmer_filter* f, int64_t* words, void** d_seen, void** d_twice)
{
    if (!f) return fail(KBBQ_E_ARG, "kbbq_kmer_filter_info: filter is NULL");
    if (words) *words = f->words;
    if (d_seen) *d_seen = f->seen;
    if (d_twice) *d_twice = f->twice;
    return KBBQ_OK;
}

int kbbq_kmer_filter_admitted(kbbq_ctx* c, const kbbq_kmer_filter* f, int64_t* admitted)
{
    if (!c || !f || !admitted) return fail(KBBQ_E_ARG, "kbbq_kmer_filter_admitted: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    u64 v = 0;
    HIPCHK(hipMemcpyAsync(&v, f->admitted, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *admitted = (int64_t)v;
    return KBBQ_OK;
}

static KmerFilterParams kmer_filter_params(const kbbq_kmer_filter* f)
{
    KmerFilterParams q;
    q.seen = f->seen; q.twice = f->twice; q.wmask = (u64)f->words - 1; q.admitted = f->admitted;
    return q;
}

static int kmer_prefilter_rows(kbbq_ctx* c, const char* who, kbbq_kmer_filter* f, int k, const uint8_t* d_seq, const uint32_t* d_meta,
                               int64_t n, int pitch, bool nib)
{
    if (!c || !f) return fail(KBBQ_E_ARG, "%s: NULL ctx or filter", who);
    if (k < 8 || k > 32) return fail(KBBQ_E_ARG, "%s: k must be in 8..32, got %d", who, k);
    if (!f->seen) return fail(KBBQ_E_ARG, "%s: the filter's `seen` array has been released", who);
    KmerParams p; size_t lds = 0;
    int rc = kmer_rows(c, who, k, d_seq, d_meta, n, pitch, nib, KM_LDS_PREFILTER, 1, p, &lds);
    if (rc || n == 0) return rc;
    const KmerFilterParams fp = kmer_filter_params(f);
    return kmer_launches(c, p, KM_READER(km_prefilter, nib), lds, &fp);
}

int kbbq_kmer_prefilter_dev(kbbq_ctx* c, kbbq_kmer_filter* f, int k, const uint8_t* d_seq, const uint32_t* d_meta, int64_t n, int pitch)
{
    return kmer_prefilter_rows(c, "kbbq_kmer_prefilter_dev", f, k, d_seq, d_meta, n, pitch, false);
}

int kbbq_kmer_prefilter_rows_dev(kbbq_ctx* c, kbbq_kmer_filter* f, int k, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                                 int pitch, int flags)
{
    bool nib = false;
    int rc = kmer_row_flags("kbbq_kmer_prefilter_rows_dev", flags, &nib);
    if (rc) return rc;
    return kmer_prefilter_rows(c, "kbbq_kmer_prefilter_rows_dev", f, k, d_seq, d_meta, nrows, pitch, nib);
}

// parts == 1: km_count_filtered itself; else km_count_filtered_part
static int kmer_count_filtered_rows(kbbq_ctx* c, const char* who, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* d_seq,
                                    const uint32_t* d_meta, int64_t n, int pitch, bool nib, int parts = 1, int part = 0)
{
    int rc = kmer_part_ok(who, parts, part);
    if (rc) return rc;
    if (!f) return fail(KBBQ_E_ARG, "%s: filter is NULL", who);
    KmerParams p; size_t lds = 0;
    rc = kmer_geometry(c, who, t, d_seq, d_meta, n, pitch, nib, KM_LDS_COUNT, 1, p, &lds);
    if (rc || n == 0) return rc;
    const KmerFilterParams fp = kmer_filter_params(f);
    if (parts == 1) return kmer_launches(c, p, KM_READER(km_count_filtered, nib), lds, &fp);
    const KmerPartParams pp = {(u32)parts, (u32)part};
    return kmer_launches(c, p, KM_READER(km_count_filtered_part, nib), lds, &fp, nullptr, &pp);
}

int kbbq_kmer_count_filtered_dev(kbbq_ctx* c, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* d_seq,
                                 const uint32_t* d_meta, int64_t n, int pitch)
{
    return kmer_count_filtered_rows(c, "kbbq_kmer_count_filtered_dev", t, f, d_seq, d_meta, n, pitch, false);
}

int kbbq_kmer_count_filtered_rows_dev(kbbq_ctx* c, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* d_seq,
                                      const uint32_t* d_meta, int64_t nrows, int pitch, int flags)
{
    bool nib = false;
    int rc = kmer_row_flags("kbbq_kmer_count_filtered_rows_dev", flags, &nib);
    if (rc) return rc;
    return kmer_count_filtered_rows(c, "kbbq_kmer_count_filtered_rows_dev", t, f, d_seq, d_meta, nrows, pitch, nib);
}

int kbbq_kmer_count_filtered_part_dev(kbbq_ctx* c, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* d_seq,
                                      const uint32_t* d_meta, int64_t n, int pitch, int parts, int part)
{
    return kmer_count_filtered_rows(c, "kbbq_kmer_count_filtered_part_dev", t, f, d_seq, d_meta, n, pitch, false, parts, part);
}

int kbbq_kmer_count_filtered_rows_part_dev(kbbq_ctx* c, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* d_seq,
                                           const uint32_t* d_meta, int64_t nrows, int pitch, int flags, int parts, int part)
{
    bool nib = false;
    int rc = kmer_part_ok("kbbq_kmer_count_filtered_rows_part_dev", parts, part);
    if (!rc) rc = kmer_row_flags("kbbq_kmer_count_filtered_rows_part_dev", flags, &nib);
    if (rc) return rc;
    return kmer_count_filtered_rows(c, "kbbq_kmer_count_filtered_rows_part_dev", t, f, d_seq, d_meta, nrows, pitch, nib, parts, part);
}

int kbbq_kmer_prefilter(kbbq_ctx* c, kbbq_kmer_filter* f, int k, const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch)
{
    if (!c || !f) return fail(KBBQ_E_ARG, "kbbq_kmer_prefilter: NULL ctx or filter");
    if (n < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "kbbq_kmer_prefilter: bad n/pitch");
    if (n > 0 && (!seq || !meta)) return fail(KBBQ_E_ARG, "kbbq_kmer_prefilter: NULL plane");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    // a slab: seq | meta
    return stage_run(c, "kbbq_kmer_prefilter", {seq}, meta, nullptr, n, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kbbq_kmer_prefilter_dev(c, f, k, d, (const uint32_t*)(d + plane), m, pitch);
    });
}

static int kmer_count_filtered_host(kbbq_ctx* c, const char* who, const char* dev, kbbq_kmer_table* t, const kbbq_kmer_filter* f,
                                    const uint8_t* seq, const uint32_t* meta, int64_t n, int pitch, int parts, int part)
{
    int rc = kmer_part_ok(who, parts, part);
    if (rc) return rc;
    if (!c || !t || !f) return fail(KBBQ_E_ARG, "%s: NULL ctx, table or filter", who);
    if (n < 0 || pitch <= 0 || (pitch & 15)) return fail(KBBQ_E_ARG, "%s: bad n/pitch", who);
    if (n > 0 && (!seq || !meta)) return fail(KBBQ_E_ARG, "%s: NULL plane", who);
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    return stage_run(c, who, {seq}, meta, nullptr, n, pitch, [&](uint8_t* d, size_t plane, int64_t m) {
        return kmer_count_filtered_rows(c, dev, t, f, d, (const uint32_t*)(d + plane), m, pitch, false, parts, part);
    });
}

int kbbq_kmer_count_filtered(kbbq_ctx* c, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* seq, const uint32_t* meta,
                             int64_t n, int pitch)
{
    return kmer_count_filtered_host(c, "kbbq_kmer_count_filtered", "kbbq_kmer_count_filtered_dev", t, f, seq, meta, n, pitch, 1, 0);
}

int kbbq_kmer_count_filtered_part(kbbq_ctx* c, kbbq_kmer_table* t, const kbbq_kmer_filter* f, const uint8_t* seq, const uint32_t* meta,
                                  int64_t n, int pitch, int parts, int part)
{
    return kmer_count_filtered_host(c, "kbbq_kmer_count_filtered_part", "kbbq_kmer_count_filtered_part_dev", t, f, seq, meta, n, pitch,
                                    parts, part);
}

} // extern "C"

// ---- BGZF output (csrc/kbbq_bgzf.h) -------------------------------------------------------------------------------------------
static int64_t bgzf_blocks_of(int64_t n, int block_bytes) { return (n + block_bytes - 1) / block_bytes; }

static int bgzf_block_bytes_ok(const char* who, int block_bytes)
{
    if (block_bytes < 1 || block_bytes > (int)BZ_MAX_TEXT)
        return fail(KBBQ_E_ARG, "%s: block_bytes %d is not in 1..%u", who, block_bytes, BZ_MAX_TEXT);
    return KBBQ_OK;
}

// the launches of one piece of text (n > 0, arguments checked): blocks, sizes, offsets, packed bytes; the packed length is left
// in c->bgzf_off[nblocks]
static int bgzf_launch(kbbq_ctx* c, const uint8_t* d_text, int64_t n, int block_bytes, uint8_t* d_blocks, uint32_t* d_sizes,
                       uint8_t* d_packed)
{
    const int64_t nb = bgzf_blocks_of(n, block_bytes);
    const unsigned grid = (unsigned)std::min<int64_t>(nb, std::max(c->cus, 1));
    int rc = grow_scratch(c, c->bgzf_tok, (size_t)grid * BZ_MAX_TEXT * sizeof(u32));
    if (!rc) rc = grow_scratch(c, c->bgzf_off, (size_t)(nb + 1) * sizeof(u64));
    if (rc) return rc;
    BgzfParams q{d_text, n, (u32)block_bytes, (u32)nb, d_blocks, d_sizes, (u32*)c->bgzf_tok.p};
    void* args[] = {&q};
    (void)hipLaunchKernel(LDS_KERNELS[LK_BGZF], dim3(grid), dim3(BZ_THREADS), args, BZ_LDS_BYTES, c->stream);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(bz_scan_sizes, dim3(1), dim3(BZ_THREADS), 0, c->stream, (const u32*)d_sizes, (u32)nb, (u64*)c->bgzf_off.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(bz_pack, dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint8_t*)d_blocks, (const u32*)d_sizes,
                       (const u64*)c->bgzf_off.p, d_packed);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

extern "C" {

size_t kbbq_bgzf_bound(int64_t n, int block_bytes)
{
    if (n <= 0 || block_bytes < 1 || block_bytes > (int)BZ_MAX_TEXT) return 0;
    return (size_t)n + 31 * (size_t)bgzf_blocks_of(n, block_bytes);
}

int kbbq_bgzf_eof(uint8_t* out)
{
    static const uint8_t eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0,
                                    0, 0, 0, 0, 0, 0, 0, 0};
    if (!out) return fail(KBBQ_E_ARG, "kbbq_bgzf_eof: out is NULL");
    memcpy(out, eof, sizeof eof);
    return KBBQ_OK;
}

int kbbq_bgzf_deflate_dev(kbbq_ctx* c, const uint8_t* d_text, int64_t n, int block_bytes, uint8_t* d_blocks, uint32_t* d_sizes,
                          uint8_t* d_packed, size_t* packed_bytes)
{
    int rc = bgzf_block_bytes_ok("kbbq_bgzf_deflate_dev", block_bytes);
    if (rc) return rc;
    if (!c || !packed_bytes) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: NULL ctx or packed_bytes");
    *packed_bytes = 0;
    if (n < 0) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: n < 0");
    if (n == 0) return KBBQ_OK;
    if (!d_text || !d_blocks || !d_sizes || !d_packed) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: NULL buffer");
    if (((uintptr_t)d_blocks & 3) || ((uintptr_t)d_sizes & 3)) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: d_blocks and d_sizes are 4-byte aligned");
    if (bgzf_blocks_of(n, block_bytes) > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate_dev: more than 2^31 - 1 blocks");
    HIPCHK(hipSetDevice(c->device));
    rc = bgzf_launch(c, d_text, n, block_bytes, d_blocks, d_sizes, d_packed);
    if (rc) return rc;
    u64 total = 0;
    HIPCHK(hipMemcpyAsync(&total, (const u64*)c->bgzf_off.p + bgzf_blocks_of(n, block_bytes), sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *packed_bytes = (size_t)total;
    return KBBQ_OK;
}

int kbbq_bgzf_deflate(kbbq_ctx* c, const uint8_t* text, int64_t n, int block_bytes, uint8_t* out, size_t out_cap, size_t* out_bytes)
{
    int rc = bgzf_block_bytes_ok("kbbq_bgzf_deflate", block_bytes);
    if (rc) return rc;
    if (!c || !out_bytes) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: NULL ctx or out_bytes");
    *out_bytes = 0;
    if (n < 0) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: n < 0");
    if (n == 0) return KBBQ_OK;
    if (!text || !out) return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: NULL buffer");
    if (out_cap < kbbq_bgzf_bound(n, block_bytes))
        return fail(KBBQ_E_ARG, "kbbq_bgzf_deflate: out holds %zu bytes, kbbq_bgzf_bound is %zu", out_cap, kbbq_bgzf_bound(n, block_bytes));
    HIPCHK(hipSetDevice(c->device));
    // a slab: `per` blocks.  Host: text | packed | packed length; device: text | packed | sizes; the blocks before packing in
    // scratch of the context's.  While the kernels of slab k run, the host copies slab k + 1 in and slab k - 1 out.
    const char* e = getenv("KBBQ_STAGE_MB");
    const size_t budget = (size_t)(e && atoi(e) > 0 ? atoi(e) : 96) << 20;
    const int64_t nb = bgzf_blocks_of(n, block_bytes);
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(nb, (int64_t)(budget / (3 * (size_t)BZ_SLOT))));
    const size_t text_cap = align16((size_t)per * block_bytes), packed_cap = align16((size_t)per * (block_bytes + 31));
    const size_t bytes = text_cap + packed_cap + align16((size_t)per * 4 + 8);
    rc = stage_prepare(c, bytes);
    if (!rc) rc = grow_scratch(c, c->bgzf_blocks, (size_t)per * BZ_SLOT);
    if (rc) return rc;
    size_t written = 0;
    auto finish = [&](int buf) -> int {                    // slab in `buf`: its packed bytes to `out`
        HIPCHK(hipEventSynchronize(c->stage_up[buf]));
        const u64 total = *(const u64*)((const char*)c->stage_host[buf] + text_cap + packed_cap);
        if (written + total > out_cap) return fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: more bytes than kbbq_bgzf_bound");
        HIPCHK(hipMemcpyAsync((char*)c->stage_host[buf] + text_cap, (const char*)c->stage_dev[buf] + text_cap, (size_t)total,
                              hipMemcpyDeviceToHost, c->stage_down_stream));
        HIPCHK(hipStreamSynchronize(c->stage_down_stream));
        threaded_copy(out + written, (const char*)c->stage_host[buf] + text_cap, (size_t)total);
        written += (size_t)total;
        return KBBQ_OK;
    };
    int64_t k = 0;
    for (int64_t lo = 0; lo < nb; lo += per, ++k) {
        const int buf = (int)(k & 1);
        const int64_t first = lo * block_bytes, m = std::min<int64_t>(n - first, per * block_bytes), mb = bgzf_blocks_of(m, block_bytes);
        threaded_copy(c->stage_host[buf], text + first, (size_t)m);
        uint8_t* d = (uint8_t*)c->stage_dev[buf];
        rc = hipMemcpyAsync(d, c->stage_host[buf], (size_t)m, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 ? KBBQ_OK : fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: upload failed");
        if (!rc) rc = bgzf_launch(c, d, m, block_bytes, (uint8_t*)c->bgzf_blocks.p, (uint32_t*)(d + text_cap + packed_cap), d + text_cap);
        if (!rc && hipMemcpyAsync((char*)c->stage_host[buf] + text_cap + packed_cap, (const u64*)c->bgzf_off.p + mb, sizeof(u64),
                                  hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: download failed");
        if (!rc && hipEventRecord(c->stage_up[buf], c->stream) != hipSuccess) rc = fail(KBBQ_E_HIP, "kbbq_bgzf_deflate: hipEventRecord failed");
        if (!rc && k > 0) rc = finish(buf ^ 1);
        if (rc) return stage_drain(c, rc);
    }
    rc = finish((int)((k - 1) & 1));
    if (rc) return stage_drain(c, rc);
    *out_bytes = written;
    return KBBQ_OK;
}

} // extern "C"

// ---- BGZF input (csrc/kbbq_bgzf_inflate.h) ------------------------------------------------------------------------------------
static int inflate_launch(kbbq_ctx* c, hipStream_t stream, const uint8_t* d_src, size_t src_bytes, const kbbq_bgzf_block* d_blocks,
                          int64_t nblocks, uint8_t* d_out, size_t out_bytes, uint32_t* d_status)
{
    if ((size_t)c->lds_bytes < BI_LDS_BYTES) return fail(KBBQ_E_ARG, "bi_inflate needs %zu bytes of LDS, the device has %d", BI_LDS_BYTES, c->lds_bytes);
    const unsigned grid = (unsigned)std::min<int64_t>(nblocks, std::max(c->cus, 1));
    BiParams q{d_src, (uint64_t)src_bytes, d_blocks, (uint32_t)nblocks, d_out, (uint64_t)out_bytes, d_status};
    void* args[] = {&q};
    (void)hipLaunchKernel(LDS_KERNELS[LK_BGZF_INFLATE], dim3(grid), dim3(BI_THREADS), args, BI_LDS_BYTES, stream);
    HIPCHK(hipGetLastError());
    return KBBQ_OK;
}

static int inflate_stage_prepare(kbbq_ctx* c, size_t bytes)
{
    if (!c->inflate_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->inflate_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) HIPCHK(hipEventCreateWithFlags(&c->inflate_done[b], hipEventDisableTiming));
    }
    if (c->inflate_bytes < bytes) {
        HIPCHK(hipStreamSynchronize(c->inflate_stream));
        for (int b = 0; b < 2; ++b) {
            if (c->inflate_host[b]) { (void)hipHostFree(c->inflate_host[b]); c->inflate_host[b] = nullptr; }
            if (c->inflate_dev[b]) { (void)hipFree(c->inflate_dev[b]); c->inflate_dev[b] = nullptr; }
        }
        c->inflate_bytes = 0;
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipHostMalloc(&c->inflate_host[b], bytes, hipHostMallocDefault));
            HIPCHK(hipMalloc(&c->inflate_dev[b], bytes));
        }
        c->inflate_bytes = bytes;
    }
    return KBBQ_OK;
}

// The members of an indexed stream (kbbq_inflate_index) into out, slab by slab of whole members; members the kernel gave a status are
// inflated again by kbbq_inflate_blocks_host.  *data_error: that failed too -- the input is damaged, the text is in the error.
static int kbbq_inflate_bgzf_indexed_(kbbq_ctx* c, const uint8_t* src, size_t n, const kbbq_bgzf_block* blocks, size_t nblocks, uint8_t* out,
                                      kbbq_inflate_stats* stats, bool* data_error)
{
    *data_error = false;
    kbbq_inflate_stats st = {0, 0, 0, 0};
    if (stats) *stats = st;
    if (!nblocks) return KBBQ_OK;
    std::lock_guard<std::mutex> guard(c->inflate_lock);
    HIPCHK(hipSetDevice(c->device));
    // a slab: up to `per` members.  Host and device alike: compressed bytes | descriptors | status words | text
    const char* e = getenv("KBBQ_STAGE_MB");
    const size_t budget = (size_t)(e && atoi(e) > 0 ? atoi(e) : 96) << 20;
    const size_t per = std::max<size_t>(1, std::min<size_t>(nblocks, budget / (2 * (size_t)BI_MAX_TEXT + 64)));
    const size_t o_blocks = align16(per * (size_t)BI_MAX_PAYLOAD), o_status = o_blocks + per * sizeof(kbbq_bgzf_block);
    const size_t o_text = align16(o_status + per * 4), bytes = o_text + per * (size_t)BI_MAX_TEXT;
    int rc = inflate_stage_prepare(c, bytes);
    if (rc) return rc;
    hipStream_t s = c->inflate_stream;
    std::vector<uint32_t> again;                           // members for the host
    struct Slab { size_t lo, hi; } slab[2] = {{0, 0}, {0, 0}};
    auto finish = [&](int buf) -> int {                    // the slab in `buf`: its text to `out`, its refused members to `again`
        HIPCHK(hipEventSynchronize(c->inflate_done[buf]));
        const size_t lo = slab[buf].lo, hi = slab[buf].hi;
        const size_t text = (size_t)(blocks[hi - 1].dst + blocks[hi - 1].isize - blocks[lo].dst);
        threaded_copy(out + blocks[lo].dst, (const char*)c->inflate_host[buf] + o_text, text);
        const uint32_t* status = (const uint32_t*)((const char*)c->inflate_host[buf] + o_status);
        for (size_t b = lo; b < hi; ++b) if (status[b - lo]) again.push_back((uint32_t)b);
        st.bytes_down += text + (hi - lo) * 4;
        return KBBQ_OK;
    };
    size_t k = 0;
    for (size_t lo = 0; lo < nblocks; ++k) {
        const int buf = (int)(k & 1);
        const size_t hi = std::min(nblocks, lo + per);
        const size_t base = (size_t)blocks[lo].src, comp = (size_t)(blocks[hi - 1].src + blocks[hi - 1].csize) - base;
        const size_t text = (size_t)(blocks[hi - 1].dst + blocks[hi - 1].isize - blocks[lo].dst);
        if (comp > per * (size_t)BI_MAX_PAYLOAD || text > per * (size_t)BI_MAX_TEXT || base + comp > n)
            { rc = fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: the block table does not describe BGZF members"); break; }
        if (k >= 2) { rc = finish(buf); if (rc) break; }   // the slab that used this buffer
        char* h = (char*)c->inflate_host[buf];
        char* d = (char*)c->inflate_dev[buf];
        threaded_copy(h, src + base, comp);
        kbbq_bgzf_block* hb = (kbbq_bgzf_block*)(h + o_blocks);
        for (size_t b = lo; b < hi; ++b) {
            hb[b - lo] = blocks[b];
            hb[b - lo].src -= base; hb[b - lo].dst -= blocks[lo].dst;
        }
        slab[buf] = Slab{lo, hi};
        if (hipMemcpyAsync(d, h, comp, hipMemcpyHostToDevice, s) != hipSuccess
            || hipMemcpyAsync(d + o_blocks, h + o_blocks, (hi - lo) * sizeof(kbbq_bgzf_block), hipMemcpyHostToDevice, s) != hipSuccess)
            rc = fail(KBBQ_E_HIP, "kbbq_inflate_bgzf: upload failed");
        if (!rc) rc = inflate_launch(c, s, (const uint8_t*)d, comp, (const kbbq_bgzf_block*)(d + o_blocks), (int64_t)(hi - lo),
                                     (uint8_t*)d + o_text, text, (uint32_t*)(d + o_status));
        if (!rc && (hipMemcpyAsync(h + o_status, d + o_status, (hi - lo) * 4, hipMemcpyDeviceToHost, s) != hipSuccess
                    || (text && hipMemcpyAsync(h + o_text, d + o_text, text, hipMemcpyDeviceToHost, s) != hipSuccess)))
            rc = fail(KBBQ_E_HIP, "kbbq_inflate_bgzf: download failed");
        if (!rc && hipEventRecord(c->inflate_done[buf], s) != hipSuccess) rc = fail(KBBQ_E_HIP, "kbbq_inflate_bgzf: hipEventRecord failed");
        if (rc) break;
        st.bytes_up += comp + (hi - lo) * sizeof(kbbq_bgzf_block);
        lo = hi;
    }
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    if (k >= 2) rc = finish((int)(k & 1));
    if (!rc) rc = finish((int)((k - 1) & 1));
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    st.device_blocks = nblocks - again.size(); st.host_blocks = again.size();
    if (stats) *stats = st;
    if (!again.empty()) {
        std::string err;
        if (!kbbq_inflate_blocks_host(src, blocks, again.data(), again.size(), out, again.size() << 14, err)) { *data_error = true; return fail(KBBQ_E_ARG, "%s", err.c_str()); }
    }
    return KBBQ_OK;
}

extern "C" {

int kbbq_inflate_bgzf_dev(kbbq_ctx* c, const uint8_t* d_src, size_t src_bytes, const kbbq_bgzf_block* d_blocks, int64_t nblocks,
                          uint8_t* d_out, size_t out_bytes, uint32_t* d_status)
{
    if (!c) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: NULL ctx");
    if (nblocks < 0 || nblocks > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: nblocks must be in 0..2^31 - 1");
    if (nblocks == 0) return KBBQ_OK;
    if (!d_blocks || !d_status || (src_bytes && !d_src) || (out_bytes && !d_out)) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: NULL buffer");
    if (((uintptr_t)d_blocks & 7) || ((uintptr_t)d_status & 3))
        return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_dev: d_blocks is 8-byte and d_status 4-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    int rc = inflate_launch(c, c->stream, d_src, src_bytes, d_blocks, nblocks, d_out, out_bytes, d_status);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_inflate_bgzf(kbbq_ctx* c, const uint8_t* src, size_t n, uint8_t* out, size_t out_cap, size_t* text_bytes,
                      kbbq_inflate_stats* stats)
{
    if (!c || !text_bytes) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: NULL ctx or text_bytes");
    *text_bytes = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return KBBQ_OK;
    if (!src) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: NULL buffer");
    size_t nb = 0, total = 0;
    int rc = kbbq_inflate_index(src, n, nullptr, 0, &nb, &total);
    if (rc == KBBQ_INFLATE_NOT_BGZF) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: the input is not BGZF");
    if (rc) return rc;
    if (total > out_cap || (total && !out)) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf: out holds %zu bytes, the text is %zu", out_cap, total);
    std::vector<kbbq_bgzf_block> blocks(nb);
    rc = kbbq_inflate_index(src, n, blocks.data(), nb, &nb, &total);
    if (rc) return rc;
    bool data_error = false;
    rc = kbbq_inflate_bgzf_indexed_(c, src, n, blocks.data(), nb, out, stats, &data_error);
    if (!rc) *text_bytes = total;
    return rc;
}

int kbbq_inflate_use_ctx(kbbq_ctx* c)
{
    kbbq_inflate_set_route_(c, c ? &kbbq_inflate_bgzf_indexed_ : nullptr);
    return KBBQ_OK;
}

int kbbq_inflate_bgzf_host(const uint8_t* payload, uint32_t n, uint8_t* out, uint32_t isize, uint32_t crc)
{
    if ((n && !payload) || (isize && !out)) return fail(KBBQ_E_ARG, "kbbq_inflate_bgzf_host: NULL buffer");
    std::unique_ptr<BiTables> t(new BiTables);
    static uint8_t none[4];
    return (int)bi_member_host(payload ? payload : none, n, out ? out : none, isize, crc, t.get());
}

} // extern "C"

// ---- BAM output (csrc/kbbq_bam_out.h) -----------------------------------------------------------------------------------------
static int bam_assemble_args(const char* who, const void* skel, const void* desc, int64_t n, const void* seq, int pitch, const void* stream,
                             int64_t* bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!bad_row) return fail(KBBQ_E_ARG, "%s: bad_row is NULL", who);
    if (n < 0 || n > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "%s: n must be in 0..2^31 - 1", who);
    if (pitch <= 0 || (pitch & 15) || pitch > 65536) return fail(KBBQ_E_ARG, "%s: pitch must be a positive multiple of 16 (<= 65536), got %d", who, pitch);
    if (n > 0 && (!skel || !desc || !stream)) return fail(KBBQ_E_ARG, "%s: NULL buffer", who);
    if ((uintptr_t)seq & 15) return fail(KBBQ_E_ARG, "%s: planes must be 16-byte aligned", who);
    if ((uintptr_t)desc & 3) return fail(KBBQ_E_ARG, "%s: the descriptors must be 4-byte aligned", who);
    return KBBQ_OK;
}

extern "C" {

int kbbq_bam_assemble_dev(kbbq_ctx* c, const uint8_t* d_skel, size_t skel_bytes, const kbbq_bam_desc* d_desc, int64_t n,
                          const uint8_t* d_seq, const uint8_t* d_qplane, int pitch, uint8_t* d_stream, size_t carry,
                          size_t stream_bytes, int64_t* bad_row)
{
    int rc = bam_assemble_args("kbbq_bam_assemble_dev", d_skel, d_desc, n, d_seq, pitch, d_stream, bad_row);
    if (rc) return rc;
    if ((uintptr_t)d_qplane & 15) return fail(KBBQ_E_ARG, "kbbq_bam_assemble_dev: planes must be 16-byte aligned");
    if (!c) return fail(KBBQ_E_ARG, "kbbq_bam_assemble_dev: ctx is NULL");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    rc = grow_scratch(c, c->bam_words, 2 * sizeof(u32));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->bam_words.p, 0xFF, 2 * sizeof(u32), c->stream));
    BoParams p{d_skel, d_desc, d_seq, d_qplane, d_stream, (u64)skel_bytes, (u64)carry, (u64)stream_bytes, (u32)n, (u32)pitch,
               (u32*)c->bam_words.p};
    const unsigned grid = (unsigned)((n + BO_RECORDS - 1) / BO_RECORDS);
    hipLaunchKernelGGL(kbo_assemble, dim3(grid), dim3(BO_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    u32 words[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(words, c->bam_words.p, sizeof words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (words[1] != ~0u) return fail(KBBQ_E_ARG, "kbbq_bam_assemble_dev: the descriptor of row %u reaches outside the skeleton, the stream or its row", words[1]);
    if (words[0] != ~0u) *bad_row = (int64_t)words[0];
    return KBBQ_OK;
}

int kbbq_bam_assemble(const uint8_t* skel, size_t skel_bytes, const kbbq_bam_desc* desc, int64_t n, const uint8_t* seq,
                      const uint8_t* qplane, int pitch, uint8_t* stream, size_t carry, size_t stream_bytes, int64_t* bad_row)
{
    int rc = bam_assemble_args("kbbq_bam_assemble", skel, desc, n, nullptr, pitch, stream, bad_row);
    if (rc) return rc;
    uint8_t map[256];
    for (int k = 0; k < 256; ++k) map[k] = bo_seq_code((uint32_t)k);
    for (int64_t r = 0; r < n; ++r)
        if (!bo_fits(desc[r], skel_bytes, carry, stream_bytes, (uint32_t)pitch))
            return fail(KBBQ_E_ARG, "kbbq_bam_assemble: the descriptor of row %lld reaches outside the skeleton, the stream or its row", (long long)r);
    std::vector<int64_t> lowest(kbbq_threads_for((size_t)n * 256), -1);
    kbbq_parallel_parts((size_t)n, (unsigned)lowest.size(), [&](unsigned t, size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) {
            const size_t row = r * (size_t)pitch;
            if (bo_record(desc[r], skel, seq ? seq + row : nullptr, qplane ? qplane + row : nullptr, map, stream + carry, 0, 1) && lowest[t] < 0)
                lowest[t] = (int64_t)r;
        }
    });
    for (int64_t v : lowest) if (v >= 0 && (*bad_row < 0 || v < *bad_row)) *bad_row = v;
    return KBBQ_OK;
}

} // extern "C"

// ---- BAM index (csrc/kbbq_bam_index.h) ----------------------------------------------------------------------------------------
static int bam_index_args(const char* who, const void* skel, const void* desc, int64_t n, int depth, const void* lin_off, int n_ref,
                          const void* linear, const void* runs, int64_t cap, int64_t* n_runs, int64_t* bad_row)
{
    if (bad_row) *bad_row = -1;
    if (n_runs) *n_runs = 0;
    if (!bad_row || !n_runs) return fail(KBBQ_E_ARG, "%s: NULL result pointer", who);
    if (n < 0 || n > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "%s: n must be in 0..2^31 - 1", who);
    if (depth < 5 || depth > 8) return fail(KBBQ_E_ARG, "%s: depth must be in 5..8, got %d", who, depth);
    if (n_ref < 0) return fail(KBBQ_E_ARG, "%s: n_ref is negative", who);
    if (n > 0 && (!skel || !desc || !lin_off || !runs || (n_ref > 0 && !linear))) return fail(KBBQ_E_ARG, "%s: NULL buffer", who);
    if (cap < n) return fail(KBBQ_E_ARG, "%s: room for %lld runs, a slab of %lld records can need as many", who, (long long)cap, (long long)n);
    if ((uintptr_t)desc & 3) return fail(KBBQ_E_ARG, "%s: the descriptors must be 4-byte aligned", who);
    if (((uintptr_t)lin_off | (uintptr_t)linear | (uintptr_t)runs) & 7) return fail(KBBQ_E_ARG, "%s: lin_off, linear and runs must be 8-byte aligned", who);
    return KBBQ_OK;
}

static constexpr const char* BAM_INDEX_NO_FIT = "%s: row %lld does not fit (its head outside the skeleton, its CIGAR outside its head, "
                                                "a refID beyond the references, or an end beyond 2^(14 + 3 * depth))";

extern "C" {

int kbbq_bam_index_dev(kbbq_ctx* c, const uint8_t* d_skel, size_t skel_bytes, const kbbq_bam_desc* d_desc, int64_t n,
                       uint64_t stream_base, int depth, const uint64_t* d_lin_off, int n_ref, uint64_t* d_linear,
                       kbbq_bam_run* runs, int64_t cap, int64_t* n_runs, int64_t* bad_row)
{
    int rc = bam_index_args("kbbq_bam_index_dev", d_skel, d_desc, n, depth, d_lin_off, n_ref, d_linear, runs, cap, n_runs, bad_row);
    if (rc) return rc;
    if (!c) return fail(KBBQ_E_ARG, "kbbq_bam_index_dev: ctx is NULL");
    if (n == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    // scratch: [words 4 x u32 | lin_total u64 | key u64 n | runs 32 n | length u32 n | head_row u32 n | head_unm u32 n | block uint2]
    const size_t nb = ((size_t)n + BIX_THREADS - 1) / BIX_THREADS;
    const size_t at_key = 32, at_runs = at_key + 8 * (size_t)n, at_len = at_runs + sizeof(kbbq_bam_run) * (size_t)n,
                 at_row = at_len + 4 * (size_t)n, at_unm = at_row + 4 * (size_t)n, at_block = (at_unm + 4 * (size_t)n + 7) / 8 * 8;
    rc = grow_scratch(c, c->bam_index, at_block + sizeof(uint2) * nb);
    if (rc) return rc;
    uint8_t* s = (uint8_t*)c->bam_index.p;
    uint64_t lin_total = 0;
    HIPCHK(hipMemcpyAsync(&lin_total, d_lin_off + n_ref, sizeof lin_total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemsetAsync(s, 0xFF, sizeof(u32), c->stream));
    HIPCHK(hipMemsetAsync(s + sizeof(u32), 0, 3 * sizeof(u32), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    BixParams p{d_skel, d_desc, d_lin_off, d_linear, (u64)skel_bytes, (u64)stream_base, lin_total, (u32)n, (u32)n_ref, depth,
                (uint64_t*)(s + at_key), (u32*)(s + at_len), (uint2*)(s + at_block), (u32*)(s + at_row), (u32*)(s + at_unm),
                (kbbq_bam_run*)(s + at_runs), (u32*)s};
    hipLaunchKernelGGL(kbi_entries, dim3((unsigned)nb), dim3(BIX_THREADS), 0, c->stream, p);
    hipLaunchKernelGGL(kbi_count, dim3((unsigned)nb), dim3(BIX_THREADS), 0, c->stream, p);
    hipLaunchKernelGGL(kbi_scan, dim3(1), dim3(BIX_THREADS), 0, c->stream, p, (u32)nb);
    hipLaunchKernelGGL(kbi_heads, dim3((unsigned)nb), dim3(BIX_THREADS), 0, c->stream, p);
    hipLaunchKernelGGL(kbi_runs, dim3((unsigned)nb), dim3(BIX_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    u32 words[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(words, s, sizeof words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (words[0] != ~0u) {
        *bad_row = (int64_t)words[0];
        return fail(KBBQ_E_ARG, BAM_INDEX_NO_FIT, "kbbq_bam_index_dev", (long long)words[0]);
    }
    if (words[1] == 0 || (int64_t)words[1] > n) return fail(KBBQ_E_HIP, "kbbq_bam_index_dev: %u runs of %lld records", words[1], (long long)n);
    HIPCHK(hipMemcpyAsync(runs, s + at_runs, sizeof(kbbq_bam_run) * (size_t)words[1], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_runs = (int64_t)words[1];
    return KBBQ_OK;
}

int kbbq_bam_index(const uint8_t* skel, size_t skel_bytes, const kbbq_bam_desc* desc, int64_t n, uint64_t stream_base, int depth,
                   const uint64_t* lin_off, int n_ref, uint64_t* linear, kbbq_bam_run* runs, int64_t cap, int64_t* n_runs,
                   int64_t* bad_row)
{
    int rc = bam_index_args("kbbq_bam_index", skel, desc, n, depth, lin_off, n_ref, linear, runs, cap, n_runs, bad_row);
    if (rc) return rc;
    if (n == 0) return KBBQ_OK;
    const uint64_t lin_total = lin_off[n_ref];
    std::vector<BixEntry> entries((size_t)n);
    for (int64_t r = 0; r < n; ++r)                                      // nothing is touched when a row does not fit
        if (!bix_entry(desc[r], skel, skel_bytes, depth, n_ref, entries[(size_t)r])) {
            *bad_row = r;
            return fail(KBBQ_E_ARG, BAM_INDEX_NO_FIT, "kbbq_bam_index", (long long)r);
        }
    int64_t count = 0;
    for (int64_t r = 0; r < n; ++r) {
        const BixEntry& e = entries[(size_t)r];
        const uint64_t start = stream_base + desc[r].stream_off;
        if (e.ref >= 0)
            bix_windows(e, lin_off, start, [&](uint64_t at, uint64_t v) { if (at < lin_total && v < linear[at]) linear[at] = v; });
        if (r == 0 || ((bix_key(e) ^ bix_key(entries[(size_t)r - 1])) & BIX_RUN_MASK) != 0) {
            kbbq_bam_run& run = runs[count++];
            run.ref = e.ref; run.bin = e.bin; run.beg = start; run.n_mapped = run.n_unmapped = 0;
        }
        kbbq_bam_run& run = runs[count - 1];
        run.end = start + e.length;
        ++(e.unmapped ? run.n_unmapped : run.n_mapped);
    }
    *n_runs = count;
    return KBBQ_OK;
}

} // extern "C"
