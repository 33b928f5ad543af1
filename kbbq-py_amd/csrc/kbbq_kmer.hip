// kbbq_kmer.hip -- libkbbq_hip.so: k-mer tables, prefilters and sets; counting, correcting and flagging rows; the quality gate;
// select / merge across ranks (C ABI: include/kbbq_hip.h; shared: kbbq_lib.h).
#include "kbbq_kmer.h"
#include "kbbq_kmer_set.h"
#include "kbbq_lib.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

extern "C" {

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
