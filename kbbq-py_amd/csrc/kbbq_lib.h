// kbbq_lib.h -- what the .hip units of libkbbq_hip.so share (internal: never installed, not part of the ABI).
// The units, one domain each: kbbq_context.hip (context, device memory, events, timing, status decode -- and the definitions of
// what is declared here without another owner), kbbq_hip.hip (the rows unit: the K1 / K2 launch layer, rows, pairs, layouts, bands),
// kbbq_solve.hip (K3), kbbq_aligned.hip (K4 / K5 / K6, the aligned tally, ApplyBQSR on aligned rows, the quantizer),
// kbbq_staging.hip (the page-locked staging pipeline), kbbq_kmer.hip, kbbq_bgzf.hip (deflate and inflate), kbbq_bam.hip (assemble
// and index).  A unit relies on its own kernel headers and on this file, on nothing of another unit that is not declared here.
// Every __global__ function is compiled into exactly one unit: a kernel header with a kernel that is not a template is included by
// one unit only, and a template kernel is named (instantiated) in one unit only.
#pragma once
#include "kbbq_lib_host.h"
#include "kbbq_kernels_v3.h"       // K1v3Params (K1Setup); through kbbq_helpers.h: u32 / u64, KQ / KND, the status words, lut_row_stride

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <utility>
#include <vector>

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
    DevScratch bam_recode;            // kbbq_bam_recode_dev: the status, the two sizes, the scan's workgroup sums (csrc/kbbq_bam_recode.h)
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

// one launch's pair of events while timing is on (kbbq_ctx_kernel_ms); a device buffer freed with its scope
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

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
};

// Nothing below is part of the ABI: none of it is among the library's dynamic symbols.
#pragma GCC visibility push(hidden)

// ---- errors, switches (kbbq_context.hip) ------------------------------------------------------------------------------------
// the calling thread's error text (kbbq_last_error reads it, kbbq_set_error_ sets it as it is); returns `code`
int fail(int code, const char* fmt, ...);

// an environment switch that a test or bench.py sets: is it `value`?
inline bool env_is(const char* name, const char* value) { const char* v = getenv(name); return v && !strcmp(v, value); }

#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(KBBQ_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                           \
    } while (0)

// ---- launch helpers (kbbq_context.hip) --------------------------------------------------------------------------------------
int check_planes(const char* fn, int64_t nreads, int pitch, const void* a, const void* b, const void* c);
int layout_flags_ok(const char* who, int flags, bool errbit_ok = false);
int grow_scratch(kbbq_ctx* c, DevScratch& s, size_t need);
int bounded_grid(int64_t want, const kbbq_ctx* c, int per_cu);

static u32 magic_for(int cpr) { return cpr <= 1 ? 0u : (u32)(((1ull << 32) + (u64)cpr - 1) / (u64)cpr); }

// ---- the LUT blob's parts (kbbq_lut_bytes; written by kbbq_build_lut and the solve, read by K2) ------------------------------
static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t lut_full_offset(int R, int Qt, int S2) { return align16((size_t)R * Qt * lut_row_stride(S2) * 2); }
static size_t lut_compact8_offset(int R, int Qt, int S2) { return lut_full_offset(R, Qt, S2) + align16(kbbq_full_lut_bytes(R, Qt, S2)); }
static size_t lut_compact8_bytes(int R, int Qt, int S2) { return (size_t)R * Qt * lut_row_stride(S2); }
static size_t lut_flags_offset(int R, int Qt, int S2) { return lut_compact8_offset(R, Qt, S2) + align16(lut_compact8_bytes(R, Qt, S2)); }

// ---- the K1 launch (kbbq_hip.hip): a unit that runs a K1 form fills a K1Setup and hands it to launch_k1; it names no kernel ----
enum K1Form { K1_ROWS, K1_ALIGNED, K1_ALIGNED_REF, K1_BANDS };
// what accumulate_rows would launch (kernel parameters, LDS bytes, template variant): kbbq_accumulate_bands_dev collects
// these for all length bands and launches them as ONE kernel
struct K1Setup { K1v3Params q; int dn = 0; int kj = 0; int eb = 0; size_t lds = 0; };    // dn / kj / eb: K1_VARIANTS; lds: bytes of dynamic LDS
bool k1_geometry(K1v3Params& q, const kbbq_ctx* c, int copies, int cut, int minlen);
size_t k1_lds_plan(K1v3Params& q, int dn, const kbbq_ctx* c);
int launch_k1(kbbq_ctx* c, K1Form form, const K1Setup& su, int nib);

// ---- kbbq_ctx_create: the full LDS as dynamic shared memory to every kernel a unit launches with dynamic LDS -------------------
// (each unit for the kernels of its own tables; lap(what): kbbq_ctx_create's KBBQ_CTX_DBG line for the time since the last one)
typedef std::function<void(const char*)> CtxLap;
void rows_full_lds(int lds_bytes, const CtxLap& lap);      // kbbq_hip.hip: LDS_KERNELS, K1_VARIANTS
void bgzf_full_lds(int lds_bytes, const CtxLap& lap);      // kbbq_bgzf.hip: BGZF_LDS_KERNELS

// ---- host-buffer entry points: the staging pipeline (kbbq_staging.hip) --------------------------------------------------------
// stage_run serves the row entry points; kbbq_bgzf_deflate (kbbq_bgzf.hip) moves blocks, not rows, through the same slabs and
// streams and calls stage_prepare / threaded_copy / stage_drain itself; the inflate staging copies with threaded_copy too
int stage_prepare(kbbq_ctx* c, size_t bytes);
void threaded_copy(void* dst, const void* src, size_t bytes);
int stage_drain(kbbq_ctx* c, int rc);
int stage_run(kbbq_ctx* c, const char* who, std::initializer_list<const uint8_t*> in, const uint32_t* meta, uint8_t* out,
              int64_t n, int pitch, const std::function<int(uint8_t*, size_t, int64_t)>& launch, int64_t* bad_read = nullptr,
              const std::function<bool()>& exact = nullptr,
              const std::function<void(const uint32_t*, int64_t, int64_t)>& see_meta = nullptr);

#pragma GCC visibility pop
