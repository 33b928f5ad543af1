// kbbq_bam.hip -- libkbbq_hip.so: BAM output -- records assembled on the GPU, and the BAI / CSI index of what was written --, BAM
// input -- records decoded on the GPU --, and the recode from the one to the other
// (C ABI: include/kbbq_hip.h; shared: kbbq_lib.h).
#include "kbbq_bam_out.h"
#include "kbbq_bam_index.h"
#include "kbbq_bam_in.h"
#include "kbbq_bam_recode.h"
#include "kbbq_lib.h"
#include "host_threads.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {

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

// ---- BAM input (csrc/kbbq_bam_in.h) -------------------------------------------------------------------------------------------
static int bam_decode_args(const char* who, const BdJob& J, int64_t m, int pitch, size_t slab_bytes, const uint32_t* any_status)
{
    if (!any_status) return fail(KBBQ_E_ARG, "%s: any_status is NULL", who);
    if (m < 0 || m > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "%s: m must be in 0..2^31 - 1", who);
    if (pitch <= 0 || (pitch & 15) || pitch > 65536) return fail(KBBQ_E_ARG, "%s: pitch must be a positive multiple of 16 (<= 65536), got %d", who, pitch);
    if (slab_bytes > (size_t)UINT32_MAX) return fail(KBBQ_E_ARG, "%s: a slab holds less than 2^32 bytes", who);
    if (m > 0 && (!J.slab || !J.rec_off)) return fail(KBBQ_E_ARG, "%s: NULL buffer", who);
    if (J.cigar && !J.cig_off) return fail(KBBQ_E_ARG, "%s: cigar without cig_off", who);
    if (J.n_rg < 0 || J.n_ref < 0 || (J.n_rg > 0 && (!J.rg_off || !J.rg_ids))) return fail(KBBQ_E_ARG, "%s: n_rg / n_ref negative, or read groups without their table", who);
    if (((uintptr_t)J.seq | (uintptr_t)J.qual | (uintptr_t)J.oq | (uintptr_t)J.words) & 15) return fail(KBBQ_E_ARG, "%s: planes and words must be 16-byte aligned", who);
    if (((uintptr_t)J.rec_off | (uintptr_t)J.rg_off | (uintptr_t)J.cig_off | (uintptr_t)J.cigar) & 3) return fail(KBBQ_E_ARG, "%s: offsets and CIGAR words must be 4-byte aligned", who);
    return KBBQ_OK;
}

int kbbq_bam_decode_dev(kbbq_ctx* c, const uint8_t* d_slab, size_t slab_bytes, const uint32_t* d_rec_off, int64_t m, int pitch,
                        const uint32_t* d_rg_off, const uint8_t* d_rg_ids, int n_rg, int n_ref, const uint32_t* d_cig_off,
                        size_t cig_cap, uint8_t* d_seq, uint8_t* d_qual, uint8_t* d_oq, kbbq_bam_words* d_words, uint32_t* d_cigar,
                        uint32_t* any_status)
{
    if (any_status) *any_status = 0;
    const BdJob J{d_slab, (u64)slab_bytes, d_rec_off, (u32)m, (u32)pitch, d_rg_off, d_rg_ids, n_rg, n_ref, d_cig_off, (u64)cig_cap,
                  d_seq, d_qual, d_oq, d_words, d_cigar};
    int rc = bam_decode_args("kbbq_bam_decode_dev", J, m, pitch, slab_bytes, any_status);
    if (rc) return rc;
    if (!c) return fail(KBBQ_E_ARG, "kbbq_bam_decode_dev: ctx is NULL");
    if (m == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    rc = grow_scratch(c, c->bam_words, 2 * sizeof(u32));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->bam_words.p, 0, sizeof(u32), c->stream));
    BdParams p{J, (u32*)c->bam_words.p};
    const unsigned grid = (unsigned)((m + BD_RECORDS - 1) / BD_RECORDS);
    hipLaunchKernelGGL(kbd_decode, dim3(grid), dim3(BD_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(any_status, c->bam_words.p, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_bam_decode(const uint8_t* slab, size_t slab_bytes, const uint32_t* rec_off, int64_t m, int pitch, const uint32_t* rg_off,
                    const uint8_t* rg_ids, int n_rg, int n_ref, const uint32_t* cig_off, size_t cig_cap, uint8_t* seq, uint8_t* qual,
                    uint8_t* oq, kbbq_bam_words* words, uint32_t* cigar, uint32_t* any_status)
{
    if (any_status) *any_status = 0;
    const BdJob J{slab, (u64)slab_bytes, rec_off, (u32)m, (u32)pitch, rg_off, rg_ids, n_rg, n_ref, cig_off, (u64)cig_cap, seq, qual, oq,
                  words, cigar};
    int rc = bam_decode_args("kbbq_bam_decode", J, m, pitch, slab_bytes, any_status);
    if (rc) return rc;
    std::vector<u32> met(kbbq_threads_for((size_t)m * 512), 0);
    kbbq_parallel_parts((size_t)m, (unsigned)met.size(), [&](unsigned t, size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) met[t] |= bd_record(J, (u32)r);
    });
    for (u32 v : met) *any_status |= v;
    return KBBQ_OK;
}

// ---- BAM recode (csrc/kbbq_bam_recode.h) -----------------------------------------------------------------------------------------
static int bam_recode_args(const char* who, const void* image, const void* rec_off, int64_t first, int64_t m, int n_ref, const void* desc,
                           const void* skel, size_t skel_cap, const void* status, size_t* skel_bytes, size_t* stream_bytes, uint32_t* any_status)
{
    if (skel_bytes) *skel_bytes = 0;
    if (stream_bytes) *stream_bytes = 0;
    if (any_status) *any_status = 0;
    if (!skel_bytes || !stream_bytes || !any_status) return fail(KBBQ_E_ARG, "%s: NULL result pointer", who);
    if (first < 0 || m < 0 || m > (int64_t)INT_MAX) return fail(KBBQ_E_ARG, "%s: first must not be negative, m must be in 0..2^31 - 1", who);
    if (n_ref < 0) return fail(KBBQ_E_ARG, "%s: n_ref is negative", who);
    if (m > 0 && (!image || !rec_off || !desc || !status)) return fail(KBBQ_E_ARG, "%s: NULL buffer", who);
    if (!skel && skel_cap) return fail(KBBQ_E_ARG, "%s: skel is NULL but skel_cap is not 0", who);
    if ((uintptr_t)rec_off & 7) return fail(KBBQ_E_ARG, "%s: rec_off must be 8-byte aligned", who);
    if (((uintptr_t)desc | (uintptr_t)status) & 3) return fail(KBBQ_E_ARG, "%s: the descriptors and status words must be 4-byte aligned", who);
    return KBBQ_OK;
}

// the sizes the scan found: may the write step run?
static int bam_recode_sizes(const char* who, uint64_t skel, uint64_t stream, const void* skel_buf, size_t skel_cap, size_t* skel_bytes,
                            size_t* stream_bytes, bool* write)
{
    *write = false;
    if (stream >= ((uint64_t)1 << 31))
        return fail(KBBQ_E_RANGE, "%s: the stream of a slab must stay below 2^31 bytes (offsets are 32 bits): fewer records per slab", who);
    *skel_bytes = (size_t)skel; *stream_bytes = (size_t)stream;
    if (!skel_buf) return KBBQ_OK;                                       // sizes, descriptors and status words only
    if (skel > (uint64_t)skel_cap) return fail(KBBQ_E_ARG, "%s: the skeleton takes %llu bytes, skel holds %llu", who, (unsigned long long)skel, (unsigned long long)skel_cap);
    *write = true;
    return KBBQ_OK;
}

int kbbq_bam_recode_dev(kbbq_ctx* c, const uint8_t* d_image, size_t image_bytes, const uint64_t* d_rec_off, int64_t first, int64_t m,
                        int set_oq, const uint8_t* d_keep, int n_ref, kbbq_bam_desc* d_desc, uint8_t* d_skel, size_t skel_cap,
                        uint32_t* d_status, size_t* skel_bytes, size_t* stream_bytes, uint32_t* any_status)
{
    const char* who = "kbbq_bam_recode_dev";
    int rc = bam_recode_args(who, d_image, d_rec_off, first, m, n_ref, d_desc, d_skel, skel_cap, d_status, skel_bytes, stream_bytes, any_status);
    if (rc) return rc;
    if (!c) return fail(KBBQ_E_ARG, "%s: ctx is NULL", who);
    if (m == 0) return KBBQ_OK;
    HIPCHK(hipSetDevice(c->device));
    // scratch: [any u32, pad | totals 2 x u64 | per scan workgroup 2 x u64]
    const size_t nb = ((size_t)m + BR_THREADS - 1) / BR_THREADS;
    rc = grow_scratch(c, c->bam_recode, 24 + 16 * nb);
    if (rc) return rc;
    uint8_t* s = (uint8_t*)c->bam_recode.p;
    HIPCHK(hipMemsetAsync(s, 0, 24, c->stream));
    BrParams p;
    p.job = BrJob{d_image, (u64)image_bytes, d_rec_off + first, (u32)m, n_ref, set_oq ? 1u : 0u, d_keep, d_desc, d_status, d_skel, 0};
    p.dec = br_decode_job(p.job);
    p.any = (u32*)s; p.total = (uint64_t*)(s + 8); p.part = (uint64_t*)(s + 24);
    const unsigned grid = (unsigned)((m + BR_RECORDS - 1) / BR_RECORDS);
    hipLaunchKernelGGL(kbr_size, dim3(grid), dim3(BR_THREADS), 0, c->stream, p);
    hipLaunchKernelGGL(kbr_sums, dim3((unsigned)nb), dim3(BR_THREADS), 0, c->stream, p);
    hipLaunchKernelGGL(kbr_scan_blocks, dim3(1), dim3(BR_THREADS), 0, c->stream, p, (u32)nb);
    hipLaunchKernelGGL(kbr_offsets, dim3((unsigned)nb), dim3(BR_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    uint64_t words[3] = {0, 0, 0};                                       // 24 bytes back: the status, the two sizes
    HIPCHK(hipMemcpyAsync(words, s, sizeof words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *any_status = (u32)words[0];
    bool write = false;
    rc = bam_recode_sizes(who, words[1], words[2], d_skel, skel_cap, skel_bytes, stream_bytes, &write);
    if (rc || !write) return rc;
    p.job.skel_bytes = words[1];
    hipLaunchKernelGGL(kbr_write, dim3(grid), dim3(BR_THREADS), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return KBBQ_OK;
}

int kbbq_bam_recode(const uint8_t* image, size_t image_bytes, const uint64_t* rec_off, int64_t first, int64_t m, int set_oq,
                    const uint8_t* keep, int n_ref, kbbq_bam_desc* desc, uint8_t* skel, size_t skel_cap, uint32_t* status,
                    size_t* skel_bytes, size_t* stream_bytes, uint32_t* any_status)
{
    const char* who = "kbbq_bam_recode";
    int rc = bam_recode_args(who, image, rec_off, first, m, n_ref, desc, skel, skel_cap, status, skel_bytes, stream_bytes, any_status);
    if (rc || m == 0) return rc;
    BrJob J{image, (u64)image_bytes, rec_off + first, (u32)m, n_ref, set_oq ? 1u : 0u, keep, desc, status, skel, 0};
    const BdJob D = br_decode_job(J);
    std::vector<u32> met(kbbq_threads_for((size_t)m * 512), 0);
    kbbq_parallel_parts((size_t)m, (unsigned)met.size(), [&](unsigned t, size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) met[t] |= br_size(J, D, (u32)r);
    });
    for (u32 v : met) *any_status |= v;
    uint64_t at_skel = 0, at_stream = 0;
    for (int64_t r = 0; r < m; ++r) {
        kbbq_bam_desc& d = desc[r];
        d.skel_off = (u32)at_skel; d.stream_off = (u32)at_stream;        // (a stream of 2^31 bytes or more is refused below)
        at_skel += br_skel_size(d); at_stream += br_stream_size(d);
    }
    bool write = false;
    rc = bam_recode_sizes(who, at_skel, at_stream, skel, skel_cap, skel_bytes, stream_bytes, &write);
    if (rc || !write) return rc;
    J.skel_bytes = at_skel;
    kbbq_parallel_parts((size_t)m, kbbq_threads_for((size_t)m * 512), [&](unsigned, size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) if (!status[r]) br_write(J, (u32)r, desc[r], 0, 1);
    });
    return KBBQ_OK;
}

} // extern "C"
