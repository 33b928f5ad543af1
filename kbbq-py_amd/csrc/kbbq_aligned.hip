// kbbq_aligned.hip -- libkbbq_hip.so: aligned reads -- K4 / K5 / K6 and the tally straight from the reads as aligned, ApplyBQSR on
// aligned rows, the quantizer (C ABI: include/kbbq_hip.h; shared: kbbq_lib.h).  The tally runs a K1 form through the launch
// layer of kbbq_hip.hip (launch_k1): no K1 kernel is named here.
#include "kbbq_aligned_kernels.h"
#include "kbbq_apply_aligned.h"
#include "kbbq_lib.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

constexpr int TALLY_K4_SHARE = 8;            // kbbq_tally_aligned_dev: K4's grid is sized for 1 / 8 of the reads

extern "C" {

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

} // extern "C"
