/*
 * kbbq_hip.h -- C ABI of libkbbq_hip.so, the MI355X (gfx950) implementation of
 * kbbq's recalibrate hot path.
 *
 * The reference (adamjorr/kbbq-py @ v1) is pure Python and has no FFI layer;
 * these entry points are what a ctypes binding of its hot-path functions binds
 * (INTEGRATION.md shows the stub).  Each entry point cites the reference code it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C, no torch types; every function returns 0 (KBBQ_OK) or a negative
 *     KBBQ_E_* code; kbbq_last_error() returns text for the calling thread.
 *   - "_dev" functions take DEVICE pointers and enqueue on the context's stream
 *     without synchronising; kernels report data errors (the reference's
 *     IndexError / TypeError cases) through the context's status word, read
 *     with kbbq_ctx_status() (which synchronises).
 *   - host-pointer functions (no suffix) stage through device memory owned by
 *     the context and synchronise before returning.
 *   - one context per device; a context is not thread-safe -- with one exception the file path relies on (kbbq/_egress.py, kbbq/_stream.py:
 *     the output pipeline copies slab k off the device while the producer thread launches K2 on slab k + 1): kbbq_dev_alloc / _free,
 *     kbbq_dev_copy_async and kbbq_event_create / _record / _sync touch nothing of the context but its stream and may be called
 *     from a second thread while the first one launches kernels and reads the status.
 *
 * Read layout ("padded SoA"): three byte planes seq / cseq / qual, one row of
 * `pitch` bytes per read, pitch a multiple of 16, rows 16-byte aligned.  Bytes
 * are the FASTQ characters (qual is phred+33).  Bytes at and beyond the read
 * length MUST be zero in the qual plane and SHOULD be 'N' in seq / cseq (any other
 * value is still handled correctly, through a slower exact check of that chunk -- or, on kbbq_apply_dev's fast route at one
 * read group, through the KBBQ_APPLY_CHECKED re-run described at kbbq_apply).
 * One uint32 of metadata per read:
 *     bits  0..15  length          (<= pitch)
 *     bits 16..30  read-group id   (first-appearance order, recalibrate.py:59-64)
 *     bit  31      second in pair  (compare_reads.py:304-306)
 *
 * Count tables: ONE int64 buffer of kbbq_tables_count(R, S2) elements,
 *     [ pos_errs[R][43][S2] | pos_total[R][43][S2] | dinuc_errs[R][43][16] | dinuc_total[R][43][16] ]
 * i.e. the four 3-D arrays of recalibrate.py:51-54 at their final size
 * (S2 = 2 * longest read).  q_* and rg_* are marginals of pos_* (SURVEY 7).
 * kbbq_accumulate* ADD into the buffer, so batches, shards and ranks compose.
 */
#ifndef KBBQ_HIP_H
#define KBBQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KBBQ_OK          0
#define KBBQ_E_HIP      -1   /* HIP runtime error (no device, out of memory, ...)        */
#define KBBQ_E_INDEX    -2   /* the reference raises IndexError on this input            */
#define KBBQ_E_TYPE     -3   /* the reference raises TypeError (base outside ACGTN)      */
#define KBBQ_E_ARG      -4   /* bad argument (alignment, sizes, read too long for LDS)   */
#define KBBQ_E_RANGE    -5   /* recalibrated quality + 33 outside 0..255     */
#define KBBQ_E_NAME     -6   /* corrected read name does not start with the read name    */
#define KBBQ_E_LUT      -7   /* a device-built LUT needs kbbq_apply_dev(KBBQ_APPLY_CHECKED)  */
#define KBBQ_E_MEANQ    -8   /* kbbq_solve_device_dev: meanq sits on a truncation boundary, solve with the host's longdouble meanq */
#define KBBQ_E_FULL     -9   /* k-mer table full: an insert found no free slot (kbbq_kmer_count*): give the table more slots */

#define KBBQ_APPLY_CHECKED 0 /* per-base range test, int16 LUT                            */
#define KBBQ_APPLY_FAST    1 /* table-driven int8 LUT, no per-base tests (LUT flags == 0) */

#define KBBQ_NQ         43   /* maxscore + 1, recalibrate.py:36                          */
#define KBBQ_NDINUC     16
#define KBBQ_ABI_VERSION 1

typedef struct kbbq_ctx kbbq_ctx;

/* ---- library / context ------------------------------------------------ */
int         kbbq_abi_version(void);
const char* kbbq_last_error(void);
int         kbbq_device_count(int* count);
/* One process per GPU (torch.distributed.run): the host threads a rank starts, and where they run.
 * kbbq_host_threads: threads the library's host stages (scan, fill, format) start for `work_bytes` of work -- at most this
 * process's SHARE of the CPUs it may use: usable CPUs / LOCAL_WORLD_SIZE (the launcher's variable; KBBQ_LOCAL_RANKS for
 * other launchers; KBBQ_HOST_THREADS overrides the ceiling), so eight ranks of one node do not start eight times the
 * host's threads.  kbbq_bind_host_to_device / _to_pci: bind the calling thread, and every thread started from it
 * afterwards, to the CPUs of the NUMA node the GPU (PCI address as hipDeviceGetPCIBusId prints it) hangs on; *numa_node
 * = -1 and nothing changed when the system names none.  The reference has no counterpart: it is single-threaded
 * (recalibrate.py:56-57,141-156 walk the reads in one Python loop).                                                    */
int         kbbq_host_threads(size_t work_bytes);
/* Ask for huge pages behind a large host buffer the caller is about to fill for the first time (madvise; a no-op where
 * transparent huge pages are off or KBBQ_HUGE_PAGES=0): the egress pipeline's render buffers.  Always KBBQ_OK. */
int         kbbq_host_advise_huge(void* p, size_t bytes);
int         kbbq_bind_host_to_pci(const char* pci_bus_id, int* numa_node, int* ncpus);
int         kbbq_bind_host_to_device(int device, int* numa_node, int* ncpus);
int         kbbq_ctx_create(int device, kbbq_ctx** out);
int         kbbq_ctx_destroy(kbbq_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream).  NULL selects the
 * device's default (null) stream -- which IS torch's current stream unless the caller
 * changed it.  A fresh context runs on a private non-blocking stream until this is called. */
int         kbbq_ctx_set_stream(kbbq_ctx* ctx, void* hip_stream);
int         kbbq_ctx_sync(kbbq_ctx* ctx);
/* Synchronise, fetch and clear the kernels' status word.  Returns KBBQ_OK or the
 * KBBQ_E_INDEX / KBBQ_E_TYPE / KBBQ_E_RANGE the reference would have raised
 * first (lowest read index; TypeError wins a tie, recalibrate.py:94 precedes
 * :114).  *read_index receives that read's index within the launch (or -1).  */
int         kbbq_ctx_status(kbbq_ctx* ctx, int64_t* read_index);
/* Device properties the host code sizes launches with.                     */
int         kbbq_ctx_info(kbbq_ctx* ctx, int* compute_units, int* lds_bytes, char* name, int name_len);

/* ---- device memory plumbing (for callers without torch) --------------- */
int kbbq_dev_alloc(kbbq_ctx* ctx, size_t bytes, void** dptr);
int kbbq_dev_free(kbbq_ctx* ctx, void* dptr);
int kbbq_dev_zero(kbbq_ctx* ctx, void* dptr, size_t bytes);                       /* async */
int kbbq_dev_upload(kbbq_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);   /* sync */
int kbbq_dev_download(kbbq_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* sync */
int kbbq_dev_mem_info(kbbq_ctx* ctx, size_t* free_bytes, size_t* total_bytes);          /* hipMemGetInfo: what the file path sizes its device budget with */
/* the rest of what the file path needs to run WITHOUT torch (kbbq/_hipmem.py: the single-GPU command line never imports
 * it): page-locked host buffers for the ingest / egress slabs, copies enqueued on the context's stream (kind 1 host to
 * device, 2 device to host, 3 device to device; no synchronisation), events on that stream (when has a slab's upload
 * left its buffer). */
int kbbq_host_alloc(size_t bytes, void** hptr);
int kbbq_host_free(void* hptr);
int kbbq_dev_copy_async(kbbq_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
int kbbq_event_create(kbbq_ctx* ctx, void** event);
int kbbq_event_record(kbbq_ctx* ctx, void* event);
int kbbq_event_sync(void* event);
int kbbq_event_destroy(void* event);

/* ---- geometry ---------------------------------------------------------- */
size_t kbbq_tables_count(int R, int S2);          /* int64 elements in a count-table buffer */
size_t kbbq_lut_count(int R, int Qt, int S2);     /* int16 elements in an apply LUT         */

/* ---- K1: error flagging + covariate binning ---------------------------
 * Replaces the loop body of recalibrate.fastq_to_covariate_arrays
 * (recalibrate.py:57-119) with find_corrected_sites (:13-20),
 * fastq_cycle_covariates / fastq_dinuc_covariates (compare_reads.py:275-302).
 * Second-in-pair cycles land on column 2*len-(i+1) (valid inputs
 * have non-decreasing lengths, so the running maximum IS the read's length).
 * q > 42 -> KBBQ_E_INDEX; a base outside ACGTN in a looked-up dinucleotide ->
 * KBBQ_E_TYPE (through kbbq_ctx_status).                                    */
int kbbq_accumulate_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq,
                        const uint8_t* d_qual, const uint32_t* d_meta,
                        int64_t nreads, int pitch, int R, int S2, int minscore,
                        int64_t* d_tables);
/* Same, with a separate quality threshold for the dinucleotide context: bases with
 * q >= minscore are counted, a context exists only where q >= dinuc_minscore.  This is
 * the rule of ReadData / CovariateData.consume_read (read.py:336-369, covariate.py:406-425:
 * `skips` decide what is counted -- the caller zeroes the quality byte of skipped bases
 * and passes minscore = 0 -- while minscore only gates the context).               */
int kbbq_accumulate_ex_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq,
                           const uint8_t* d_qual, const uint32_t* d_meta,
                           int64_t nreads, int pitch, int R, int S2, int minscore,
                           int dinuc_minscore, int64_t* d_tables);
/* The same for ONE LENGTH BAND of a mixed-length input: S2 sizes the (global) count tables as before, S_band >= the
 * longest read of THIS batch (0 = S2 / 2) sizes the kernel's LDS tables, so that short reads packed at a narrow pitch
 * use the table-driven kernel even when the input's longest read would not fit it.  Counts land in the same cells
 * (a second-in-pair column 2*len - 1 - i does not depend on the table width).  S_min: a promise that no (non-empty)
 * read of the batch is shorter (0 = no promise); long bands (~200-300 bases) need it to fit the LDS -- a cycle row
 * then has 3*S_band - S_min words -- and a read that breaks it is reported as KBBQ_E_INDEX, not counted.        */
int kbbq_accumulate_band_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                             const uint32_t* d_meta, int64_t nreads, int pitch, int R, int S2, int S_band, int S_min,
                             int minscore, int dinuc_minscore, int64_t* d_tables);
/* Host-buffer form (what a ctypes binding of the reference calls with NumPy arrays; ADDS into the four count arrays):
 * the rows travel slab by slab through page-locked staging of the context's own -- host threads copy slab k + 1 while the
 * copy engine uploads slab k and the kernel runs on slab k - 1 -- so device memory is two slabs whatever the input's size
 * (KBBQ_STAGE_MB: staging bytes per slab, default 96 MB) and the call runs at the PCIe rate of its 3 planes.  A read the
 * kernel flags is reported with its index in the WHOLE input; nothing is added to the caller's arrays then.  A read whose
 * read-group id is >= R is KBBQ_E_INDEX here (the reference indexes the group axis, recalibrate.py:111-117); the "_dev" forms
 * leave such a read uncounted without a status -- every read group walks the rows for its own reads -- so their callers keep
 * ids below R (kbbq_meta_stats_dev reports the largest).                                                               */
int kbbq_accumulate(kbbq_ctx* ctx, const uint8_t* seq, const uint8_t* cseq,
                    const uint8_t* qual, const uint32_t* meta,
                    int64_t nreads, int pitch, int R, int S2, int minscore,
                    int64_t* pos_errs, int64_t* pos_total,
                    int64_t* dinuc_errs, int64_t* dinuc_total);

/* ---- K2: delta-Q table lookup / apply ----------------------------------
 * Replaces compare_reads.recalibrate_fastq (compare_reads.py:320-328) as driven
 * by recalibrate.py:141-152.  The five model arrays are folded into one LUT blob
 * of kbbq_lut_bytes(R, Qt, S2) bytes (kbbq_build_lut on the host, kbbq_solve_dev on
 * the device):
 *   canonical part, int16, one row of kbbq_lut_row_stride(S2) entries per
 *   (read group, quality):
 *     row[0 .. S2-1]    = meanq[rg] + rgdq[rg] + qdq[rg][q] + posdq[rg][q][cycle]
 *     row[S2 .. S2+24]  = dinucdq[rg][q][d] indexed by 5*code(prev)+code(cur), codes
 *                         A0 T1 G2 C3 (compare_reads.py:199) and 4 = N / no previous
 *                         base; entries involving code 4 hold dinucdq[rg][q][-1]
 *   table-driven part, int8, indexed by the RAW quality byte (padding row, identity
 *   rows below minscore, a mirrored copy of the cycle entries for second-in-pair
 *   reads) -- see csrc/kbbq_kernels_v3.h; and an int of flags: bit 0 = a value
 *   does not fit int8, bit 1 = some (cycle, context) pair can leave 0..255.
 * new_q = cycle entry + context entry for q >= minscore, q otherwise; the output byte
 * is new_q + 33 (no clipping, compare_reads.py:327; outside 0..255 -> KBBQ_E_RANGE).
 * Cycle -(i+1) wraps on the final S2 (Python negative index).  q >= Qt, rg >= R or a
 * cycle beyond S2 -> KBBQ_E_INDEX.
 * mode KBBQ_APPLY_FAST may only be used when the blob's flags are 0 (known for a
 * host-built blob; for a device-built one kbbq_ctx_status returns KBBQ_E_LUT after
 * the fact and the caller re-runs with KBBQ_APPLY_CHECKED).                       */
int    kbbq_lut_row_stride(int S2);
size_t kbbq_full_lut_bytes(int R, int Qt, int S2);
size_t kbbq_lut_bytes(int R, int Qt, int S2);
int kbbq_build_lut(int R, int Qt, int S2, int D, int minscore,
                   const int64_t* meanq, const int64_t* rgdq, const int64_t* qdq,
                   const int64_t* posdq, const int64_t* dinucdq, void* lut_blob_out,
                   int* flags_out);
int kbbq_apply_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual,
                   const uint32_t* d_meta, int64_t nreads, int pitch,
                   int R, int Qt, int S2, int minscore,
                   const void* d_lut_blob, int mode, uint8_t* d_qual_out);
/* Host-buffer form: LUT built on the host (kbbq_build_lut), rows through the same page-locked slabs as kbbq_accumulate --
 * upload of slab k + 1, kernel on slab k and download of slab k - 1 overlap (PCIe is full duplex).  On an error status the
 * read index is that of the WHOLE input and the contents of qual_out are unspecified.
 * KBBQ_E_LUT never reaches the caller of this form.  kbbq_apply_dev(KBBQ_APPLY_FAST) with ONE read group runs a kernel that
 * only REPORTS rows it does not serve (a quality >= Qt, a letter outside ACGTN, a read longer than S2, a read group other than
 * 0, a byte other than 'N' in the seq padding of a read's last 16-byte chunk) as KBBQ_E_LUT without a read index; a caller of
 * kbbq_apply_dev re-runs with KBBQ_APPLY_CHECKED (kbbq/_device.py apply does), and kbbq_apply does so itself, over the whole
 * input: the status is then KBBQ_OK with every row's output, or the reference's KBBQ_E_INDEX / KBBQ_E_TYPE with "read N".   */
int kbbq_apply(kbbq_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint32_t* meta,
               int64_t nreads, int pitch, int R, int Qt, int S2, int D, int minscore,
               const int64_t* meanq, const int64_t* rgdq, const int64_t* qdq,
               const int64_t* posdq, const int64_t* dinucdq, uint8_t* qual_out);

/* ---- ApplyBQSR on aligned rows ----------------------------------------
 * Replaces gatk.applybqsr.recalibrate_bamread (gatk/applybqsr.py:46-78) for every alignment of a batch at once.  Rows are the
 * SAM reader's character planes (kbbq_sam_fill: SEQ, QUAL, OQ; pitch a multiple of 16, 16-byte aligned, zero padded) in
 * ALIGNED orientation, as they sit in the file; the output plane (new quality + 33, zero beyond the length) is aligned too.
 * One uint32 of metadata per row:
 *     bits  0..15  length L (0: nothing to do, the row's output is zero)
 *     bits 16..27  read-group index (< R <= 4096)
 *     bit  28      the SOURCE qualities (the ones recalibrated) are the OQ plane, else the QUAL plane
 *     bit  29      the CONTEXT qualities are the OQ plane, else the QUAL plane
 *     bit  30      reverse strand (FLAG 16)      bit 31  second in pair (FLAG 128)
 * Base i (j = i forward, L - 1 - i reverse): q = source - 33; q < minscore keeps its byte; otherwise
 *     new q = trunc(meanq[rg] + rgdq[rg] + qdq[rg][q] + dinucdq[rg][q][ctx] + posdq[rg][q][cycle])   (no clipping)
 * with cycle j (first of pair) or -(j + 1) wrapping on S2 (second), and ctx the dinucleotide in sequencing orientation from the
 * context plane with a fixed minscore of 6 (reverse rows complemented, letters other than ACGT -> N; none at j = 0, next to N or
 * below 6: column 16).  q >= Qt or j >= S2 on a recalibrated base -> KBBQ_E_INDEX; a forward row with a letter outside ACGTN
 * in a looked-up dinucleotide -> KBBQ_E_TYPE (it wins a tie); new q + 33 outside 0..255 -> KBBQ_E_RANGE; all through
 * kbbq_ctx_status with the row's index.
 * The model, `mode`:
 *   KBBQ_ALIGNED_LUT  the int16 canonical rows of kbbq_build_lut's blob (the first kbbq_lut_count(R, Qt, S2) entries; Qt <= 95):
 *                     exact for integer models, and for float models whose every truncated sum the caller has proven to be
 *                     cycle entry + context entry
 *   KBBQ_ALIGNED_F64  float64, one row of 18 + S2 doubles per (rg, q): [ meanq + rgdq + qdq (summed in that order),
 *                     dinucdq[0..16], posdq[0..S2-1] ]; the kernel evaluates (row[0] + row[1 + ctx]) + row[18 + cycle]
 *                     and truncates -- the reference's float64 sum, left to right (Qt <= 223)
 * d_qual / d_oq may be the same plane, and either may be NULL when no row selects it.                                   */
#define KBBQ_ALIGNED_LUT 0
#define KBBQ_ALIGNED_F64 1
int kbbq_apply_aligned_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint8_t* d_oq,
                           const uint32_t* d_meta, int64_t n, int pitch, int R, int Qt, int S2, int minscore,
                           const void* d_model, int mode, uint8_t* d_out);
/* Host-buffer form: the model (model_bytes bytes, as above) is uploaded once, the rows travel through the page-locked slabs of
 * kbbq_apply.  On an error *bad_read (may be NULL) receives the offending row's index in the WHOLE input, else -1.        */
int kbbq_apply_aligned(kbbq_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint8_t* oq, const uint32_t* meta,
                       int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* model, size_t model_bytes,
                       int mode, uint8_t* out, int64_t* bad_read);

/* ---- Static quantized qualities ---------------------------------------
 * `--static-quantized-quals Q[,Q...]` [--round-down-quantized] of `kbbq recalibrate` and `kbbq applybqsr`: the qualities a
 * command writes are rounded to a few levels so that the output compresses as its binned input did.  Not in the reference (its
 * quantize() is the identity); the option names follow GATK's ApplyBQSR, the rule is this project's own:
 *     levels   a non-empty set of integers minscore <= Q <= 93 (minscore: the 6 of every apply); E = sorted({minscore} U levels)
 *     the rule is a byte map qmap[256] over OUTPUT bytes b, q = b - 33  (kbbq.gatk.applybqsr.quantize_map builds it):
 *       b < 33 + minscore        qmap[b] = b: padding zeros, the separator of a mate-pair row, the bases an apply preserves, a
 *                                new quality below minscore
 *       q >= E[last]             E[last] + 33
 *       E[i] <= q < E[i + 1]     E[i] + 33 if 2q <= E[i] + E[i + 1], else E[i + 1] + 33 (nearest, ties down);
 *                                with round-down: E[i] + 33
 * Every status (KBBQ_E_RANGE of a new quality outside -33..222, KBBQ_E_INDEX, KBBQ_E_TYPE) is decided BEFORE the map, on the
 * unquantized value, with the row it is decided for today.
 * kbbq_quantize_plane_dev: d_plane[i] = d_qmap[d_plane[i]] in place over nbytes, on the context's stream -- the pass that follows
 *     K2 (kbbq_apply_dev / kbbq_apply_rows_dev / kbbq_apply_bands_dev) on any of its output planes, whatever their layout: every
 *     one is a byte plane with zero padding, and qmap[0] == 0.  nbytes a multiple of 16, d_plane 16-byte aligned (else
 *     KBBQ_E_ARG, nothing launched); nbytes == 0 is KBBQ_OK.  d_qmap: 256 bytes on the device.
 * kbbq_apply_aligned_q_dev / kbbq_apply_aligned_q: kbbq_apply_aligned_dev / kbbq_apply_aligned with the map applied, in the
 *     same kernel, to every NEW byte that passed the range check (a preserved byte is left alone: the map is the identity
 *     there).  d_qmap: 256 bytes on the device; qmap: 256 bytes on the host, uploaded once with the model.  A NULL map IS the
 *     call without _q: the same kernel, the same bytes.                                                                    */
int kbbq_quantize_plane_dev(kbbq_ctx* ctx, uint8_t* d_plane, int64_t nbytes, const uint8_t* d_qmap);
int kbbq_apply_aligned_q_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint8_t* d_oq,
                             const uint32_t* d_meta, int64_t n, int pitch, int R, int Qt, int S2, int minscore,
                             const void* d_model, int mode, uint8_t* d_out, const uint8_t* d_qmap);
int kbbq_apply_aligned_q(kbbq_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint8_t* oq, const uint32_t* meta,
                         int64_t n, int pitch, int R, int Qt, int S2, int minscore, const void* model, size_t model_bytes,
                         int mode, uint8_t* out, int64_t* bad_read, const uint8_t* qmap);

/* ---- K3: delta-Q model solve ------------------------------------------
 * Replaces compare_reads.gatk_delta_q (compare_reads.py:235-260) and, fused,
 * applybqsr.get_delta_qs (gatk/applybqsr.py:80-103).  Split of labour (DESIGN.md
 * "K3"): the host evaluates everything transcendental with the SciPy calls the
 * reference makes -- per cell comb = gammaln(n+1) - (gammaln(k+1) + gammaln(n-k+1)),
 * k = errs+1, n = total+2, and the 3 x 43 table h_consts129 = [prior_dist |
 * log p | log1p(-p)] -- and the device multiplies/adds those float64 values in
 * SciPy's order, adds the longdouble prior with an exact 80-bit emulation and
 * takes the first maximum over the 43 candidates.  Results are integers
 * identical to the reference's.
 *
 * kbbq_delta_q_dev: dq[i] = argmax_i - prior_q[i] for ncells independent cells
 * (prior_q must lie in 0..42).
 * kbbq_posterior_q_dev: the same cell solve for a float64 prior (the reference calls
 * gatk_delta_q with EstimatedQReported when it builds a report, gatk/bqsr.py:294): the
 * distance |q' - prior| is the float64 difference truncated toward zero, -1 < prior < 43;
 * returns the posterior quality argmax_i itself.
 * kbbq_solve_dev: the whole hierarchy from the device count tables: marginals,
 * read-group and quality levels (d_post_q[R*43] scratch), then cycle and
 * dinucleotide levels, writing the K2 LUT blob (kbbq_lut_bytes bytes) and, when
 * d_dq != NULL, int32 [rgdq R | qdq R*43 | posdq R*43*S2 | dinucdq R*43*17].
 * d_aux (kbbq_solve_aux_count doubles) = [comb_rg | comb_q | comb_pos | comb_dn].  */
int    kbbq_delta_q_dev(kbbq_ctx* ctx, const int64_t* d_prior_q, const int64_t* d_errs,
                        const int64_t* d_total, const double* d_comb, int64_t ncells,
                        const double* h_consts129, int64_t* d_dq);
int    kbbq_posterior_q_dev(kbbq_ctx* ctx, const double* d_prior_q, const int64_t* d_errs,
                            const int64_t* d_total, const double* d_comb, int64_t ncells,
                            const double* h_consts129, int64_t* d_post_q);
/* host helpers of the solve (no GPU): kbbq_combiln_host fills comb[i] for cells (errs[i], total[i]) with
 * the restated SciPy gammaln (csrc/solve_host.cpp; bit-identical to scipy.special.gammaln for positive
 * arguments, NaN for cells outside the distribution's support, which the solve ignores), on `threads`
 * threads; kbbq_gammaln_host exposes the gammaln itself for the tests.                              */
int    kbbq_combiln_host(const int64_t* errs, const int64_t* total, int64_t ncells, double* comb, int threads);
/* The host half of one solve in one threaded pass over the count tables as they come off the device (layout of
 * kbbq_accumulate_dev's d_tables): marg = [q_errs R*43 | q_total R*43 | rg_errs R | rg_total R] (recalibrate.py:112-115)
 * and aux = the gammaln term of every cell in kbbq_solve_dev's order [rg R | q R*43 | pos R*43*S2 | dinuc R*43*16]. */
int kbbq_solve_prep_host(const int64_t* tables, int R, int S2, double* aux, int64_t* marg, int threads);
int    kbbq_gammaln_host(const double* x, int64_t n, double* out);
/* the solve's two log tables without importing SciPy: logp[i] = xlogy(1, p[i]) = log(p[i]) and log1mp[i] = xlog1py(1, -p[i])
 * = log1p(-p[i]), both with the C library's routines, which is what SciPy 1.15 evaluates for real arguments (compared bit
 * for bit in tests/test_solve_core_host.py); the reference reaches both through scipy.stats.binom.logpmf
 * (compare_reads.py:254). */
int    kbbq_xlogy_tables_host(const double* p, int n, double* logp, double* log1mp);
/* The solve without the host (csrc/lgam_core.h): kbbq_libm_log_data reads the constants of the host libm's own log()
 * (ln 2 split in two, 5 coefficients, 128 x {1/c, log c}: 263 doubles) out of the mapped library, so that a kernel can
 * evaluate the same gammaln bit for bit; KBBQ_E_HIP when they are not found (then kbbq_solve_dev's host-fed form stays
 * in use).  kbbq_gammaln_restated_host evaluates that restatement on the host (no call into libm; x integer-valued
 * and >= 1), kbbq_gammaln_dev on the device: the caller checks either against kbbq_gammaln_host before relying on
 * kbbq_solve_device_dev.  */
int    kbbq_libm_log_data(double* out263, int count);
int    kbbq_gammaln_restated_host(const double* x, int64_t n, const double* logtab263, double* out);
int    kbbq_gammaln_dev(kbbq_ctx* ctx, const double* d_x, int64_t n, const double* d_logtab263, double* d_out);
/* kbbq_solve_dev with NOTHING from the host inside the step: marginals, the gammaln term of every cell (d_logtab263:
 * kbbq_libm_log_data's table on the device) and meanq = p_to_q(sum_q q_total[q] * 10^(-q/10) / rg_total)
 * (recalibrate.py:111,120; compare_reads.py:262-271) are formed by the kernels.  h_consts172 = the 129 model constants
 * of kbbq_solve_dev + the 43 float64 values q_to_p(q).  meanq is a TRUNCATION of a longdouble quotient in the
 * reference; the kernel forms it in double precision and, when -10 log10(mean) lies within 1e-7 of an integer (where
 * the reference's own 80-bit rounding decides; always so when a read group has one quality value only) or a read
 * group has no counted base, reports KBBQ_E_MEANQ through kbbq_ctx_status: the caller then solves through
 * kbbq_solve_dev with the host's longdouble meanq.  d_meanq_out [R] (may be NULL) receives the kernel's meanq.   */
int    kbbq_solve_device_dev(kbbq_ctx* ctx, const int64_t* d_tables, int R, int S2, int minscore,
                             const double* d_logtab263, const double* h_consts172, int32_t* d_post_q,
                             void* d_lut, int32_t* d_dq, int32_t* d_meanq_out);
size_t kbbq_solve_aux_count(int R, int S2);
size_t kbbq_solve_dq_count(int R, int S2);
int    kbbq_solve_dev(kbbq_ctx* ctx, const int64_t* d_tables, int R, int S2, int minscore,
                      const int32_t* d_meanq, const double* d_aux, const double* h_consts129,
                      int32_t* d_post_q, void* d_lut_blob, int32_t* d_dq);

/* ---- K4 / K5: benchmark-path error flagging -----------------
 * kbbq_find_errors_dev replaces compare_reads.find_read_errors (compare_reads.py:84-139)
 * for a batch of aligned reads: per read a CIGAR walk against its reference window
 * [ref_start, ref_start + ref_len) of the concatenated genome / skip-mask byte arrays
 * (skip mask = benchmark.get_full_skips, benchmark.py:22-39); cigar ops are
 * (length << 4 | op) with BAM op codes.  Outputs one byte per base (0 / 1) in the err and
 * skip planes; flip[r] != 0 reverses both for reverse-strand reads (benchmark.py:70-72).
 * A row of d_len[r] bases is written in whole 16-byte chunks, ceil(d_len[r] / 16) of them: the bytes
 * from the read's end to the end of its last chunk are 0, the chunks behind it are not touched.
 * (One exception, in a batch that fails anyway: a row of no bases whose CIGAR the reference raises
 * on takes the walk for its status and has its first chunk written as 16 zero bytes.)
 * The planes (seq, err, skip) are 16-byte aligned; genome / skipmask hold genome_len bytes each and
 * need no alignment or padding (reference windows are read with unaligned 16-byte loads, byte by
 * byte at the very end of the arrays).
 * Python's negative-index wraps of the reference (skips[-1], subset[-1]) are reproduced;
 * its IndexError / ValueError cases arrive through kbbq_ctx_status as KBBQ_E_INDEX /
 * KBBQ_E_RANGE.
 * kbbq_count_q_dev replaces the two np.bincount calls of benchmark.calculate_q
 * (benchmark.py:76-91) over the unskipped bases: counts[0..255] = observations per
 * quality (byte - qoffset), counts[256..511] = errors; ADDS into d_counts512.
 * ONE PLANE OF FLAGS: with d_skip == NULL kbbq_find_errors_dev writes both answers into d_err -- bit 0 error,
 * bit 1 skip -- and kbbq_count_q_dev / kbbq_canonical_reads_dev called with d_skip == NULL read that plane: one
 * byte per base less to write and to read when no caller wants the two boolean arrays themselves.
 * Implementation (csrc/kbbq_aligned_kernels.h): the first four CIGAR operations of every read are copied into one
 * 16-byte record per read (context-owned scratch), a lane walks them in registers and fetches the one reference
 * window its chunk needs; chunks on an operation boundary, reads with more operations and malformed input take the
 * sequential walk.                                                                             */
int kbbq_find_errors_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint32_t* d_len, int64_t nreads, int pitch,
                         const int64_t* d_ref_start, const int32_t* d_ref_len,
                         const uint32_t* d_cig_off, const uint32_t* d_cig_n, const uint32_t* d_cigar,
                         const uint8_t* d_genome, const uint8_t* d_skipmask, int64_t genome_len,
                         const uint8_t* d_flip, uint8_t* d_err, uint8_t* d_skip);
/* d_skipmask may be NULL: the reference is then FUSED -- bit 7 of every d_genome byte is that site's skip flag, the
 * low 7 bits its letter (ASCII) -- and a chunk fetches one scattered 16-byte window instead of two. */
/* kbbq_canonical_reads_dev: first half of gatk.bqsr.bam_to_bqsr_covariates (gatk/bqsr.py:52-123;
 * strand-aware covariates :23-50, skips :86-88).  Rewrites aligned reads into sequencing
 * orientation so that kbbq_accumulate_dev tallies them: per read the aligned part
 * [clip & 0xFFFF, clip >> 16) only, reverse-strand reads (flags bit 0) reverse-complemented
 * (letters outside ACGT -> N), padded to the common length S with uncounted bases; a base is
 * given quality byte 0 (never counted) when its K4 skip flag is set, its original quality is
 * below minscore, it lies in the trimmed range [trim & 0xFFFF, trim >> 16) (adaptor, host) or
 * it is N; out_cseq differs from out_seq exactly where the K4 error flag is set; out_meta =
 * S | read group (flags >> 16) << 16 | read 2 (flags bit 1) << 31.  The reference's TypeError
 * (a looked-up dinucleotide with a letter outside ACGT on a forward read, decided on the
 * ORIGINAL qualities with dinuc_minscore) arrives as KBBQ_E_TYPE.  All planes 16-byte
 * aligned, nreads * pitch bytes each, no padding rows needed.                           */
int kbbq_canonical_reads_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_err,
                             const uint8_t* d_skip, const uint32_t* d_len, const uint32_t* d_clip,
                             const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads, int pitch, int S,
                             int minscore, int dinuc_minscore, uint8_t* d_out_seq, uint8_t* d_out_cseq,
                             uint8_t* d_out_qual, uint32_t* d_out_meta);
/* The same with the layout of the output rows chosen: 0 (character planes, as above) or KBBQ_ROWS_NIBBLES -- d_out_seq /
 * d_out_cseq are then 4-bit planes of nreads * pitch / 2 bytes (the layout kbbq_accumulate_rows_dev takes with that
 * flag; one byte per base less to write here and to read there).  What the kernel needs of its input (both layouts, and
 * kbbq_canonical_reads_dev): rows are `pitch` bytes wide; a row may hold FEWER than S bases; only [clip & 0xFFFF, clip >> 16)
 * of it is read as bases and counted, and that range's upper end does not exceed the row's own length (an empty range: a row
 * of uncounted padding); bytes at or behind a row's own length are 0 in d_seq, d_oq and the flag planes.  d_len is not read:
 * every output row is S bases, the aligned part first, and out_meta says S.  A corrected base differs from its base in the low
 * bit of its code (an N: code 5 in d_out_cseq only).  Rows that cannot be packed -- a letter outside ACGTN on a forward-strand read -- make
 * kbbq_ctx_status return KBBQ_E_LUT: repeat the call with layout 0 (which is also where KBBQ_E_TYPE is decided). */
int kbbq_canonical_reads_rows_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_err,
                                  const uint8_t* d_skip, const uint32_t* d_len, const uint32_t* d_clip,
                                  const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads, int pitch, int S,
                                  int minscore, int dinuc_minscore, int layout, uint8_t* d_out_seq,
                                  uint8_t* d_out_cseq, uint8_t* d_out_qual, uint32_t* d_out_meta);
/* kbbq_accumulate_aligned_dev: kbbq_canonical_reads_rows_dev + kbbq_accumulate_rows_dev in ONE kernel (K6 fused into K1): the
 * tally of gatk.bqsr.bam_to_bqsr_covariates (gatk/bqsr.py:52-123) straight from the reads as aligned -- d_seq, d_oq (OQ
 * characters) and d_flagplane (kbbq_find_errors_dev's one plane of flags: bit 0 error, bit 1 skip) are [nreads, pitch]
 * planes of reads of at most S bases (pitch = S rounded up to 16); d_clip / d_trim / d_flags per read as for
 * kbbq_canonical_reads_dev.  What the kernel needs: rows are `pitch` bytes wide; a row may hold fewer than S bases; only
 * [clip & 0xFFFF, clip >> 16) of it is counted, and clip's upper end does not exceed the row's own length; bytes at or behind a
 * row's own length are 0 in all three planes.  The cycle of a base is its position in the aligned part in sequencing
 * orientation, c = i - (clip & 0xFFFF) or (clip >> 16) - 1 - i on the reverse strand: column c for read 1, S2 - 1 - c for read 2,
 * whatever the row's length.  Counts ADD into d_tables (R, S2 = 2 S).  3 B/base read instead of 3 + 2 written + 2 read
 * again.  A forward-strand read with a letter outside ACGTN makes kbbq_ctx_status return KBBQ_E_LUT: tally through
 * kbbq_canonical_reads_rows_dev(layout 0), where the reference's TypeError is decided; a shape whose tables do not fit the
 * LDS, and reads shorter than 32 bases, return KBBQ_E_LUT at once (nothing launched). */
int kbbq_accumulate_aligned_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_oq, const uint8_t* d_flagplane,
                                const uint32_t* d_clip, const uint32_t* d_trim, const uint32_t* d_flags, int64_t nreads,
                                int pitch, int S, int R, int minscore, int dinuc_minscore, int64_t* d_tables);
/* kbbq_tally_aligned_dev: kbbq_find_errors_dev (no flip, one plane of flags, fused reference) + kbbq_accumulate_aligned_dev --
 * the whole device side of gatk.bqsr.bam_to_bqsr_covariates (gatk/bqsr.py:52-123: compare_reads.find_read_errors per read,
 * compare_reads.py:84-139, then the covariate counts) -- with ONE pass over the reads for every read that is a single
 * M / = / X operation over all of its bases: the tally kernel compares such a read with its reference window itself (read
 * bytes, OQ, reference: 3 B/base instead of 6 for the two calls).  Every other read (insertions, deletions, clips in the
 * CIGAR, more or odd operations, a window at the very end of the genome) is listed on the device, kbbq_find_errors_dev's kernel
 * runs over the listed reads only and writes THEIR rows of d_flagplane, which the tally kernel reads for them.  d_flagplane:
 * [nreads, pitch] scratch of the caller's (contents on entry irrelevant; rows of listed reads hold their flags afterwards).
 * d_genome: FUSED reference (bit 7 of a byte = the site's skip flag), genome_len bytes.  d_len[i] == S for every read (the
 * caller's promise: kbbq_accumulate_aligned_dev takes shorter rows, this call does not).  Counts ADD into d_tables and equal those of the two calls; the
 * same statuses arrive through kbbq_ctx_status (KBBQ_E_INDEX / KBBQ_E_RANGE from the CIGAR walk, KBBQ_E_LUT for a forward
 * read with a letter outside ACGTN); a shape the tally kernel does not serve returns KBBQ_E_LUT before anything is launched. */
int kbbq_tally_aligned_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_oq, const uint32_t* d_len, int64_t nreads,
                           int pitch, int S, const int64_t* d_ref_start, const int32_t* d_ref_len,
                           const uint32_t* d_cig_off, const uint32_t* d_cig_n, const uint32_t* d_cigar,
                           const uint8_t* d_genome, int64_t genome_len,
                           const uint32_t* d_clip, const uint32_t* d_trim, const uint32_t* d_flags,
                           uint8_t* d_flagplane, int R, int minscore, int dinuc_minscore, int64_t* d_tables);
int kbbq_count_q_dev(kbbq_ctx* ctx, const uint8_t* d_qual, const uint8_t* d_err, const uint8_t* d_skip,
                     const uint32_t* d_len, int64_t nreads, int pitch, int qoffset, int64_t* d_counts512);
/* kbbq_flag_confusion_dev: the joint tally of TWO answers to "which base is an error" by reported quality -- what
 * `kbbq benchmark --kmers` prints.  d_qual, d_truth and d_kflags are [nreads, pitch] byte planes of the same rows in the same
 * orientation, 16-byte aligned, pitch a positive multiple of 16; d_len the reads' lengths.
 *   d_truth   kbbq_find_errors_dev's ONE plane of flags: bit 0 error, bit 1 skip;
 *   d_kflags  the plane of kbbq_kmer_flag_ex_dev (KBBQ_KMER_FLAG_UNRESOLVED): 0 trusted, 1 error, 2 unresolved;
 *   d_qual    quality bytes; a base's quality is byte - qoffset (33 for characters, 0 for values).
 * A base is counted when it lies inside its read (i < d_len[r]) and its skip bit is clear; it ADDS one to
 *   d_counts1536[q][e][k]   (int64 [256][2][3], C order)   e = bit 0 of the truth byte,
 *                                                           k = 1 if bit 0 of the kflags byte is set, else 2 if bit 1 is, else 0.
 * Nothing else is looked at: bytes at or beyond a read's length and bytes of skipped bases may hold anything.  A COUNTED base
 * whose byte is below qoffset is counted nowhere and makes kbbq_ctx_status return KBBQ_E_RANGE with its read, as
 * kbbq_count_q_dev does; the same byte at a skipped base or behind the read does not.
 * Summed over k the counts are kbbq_count_q_dev's: counts[q][0][*] + counts[q][1][*] its totals, counts[q][1][*] its errors.
 * ONE CALL TAKES AT MOST KBBQ_CONFUSION_MAX_BASES = 2^32 - 1 BASES (nreads * pitch): the kernel counts in 32-bit words of LDS
 * that it flushes once, and a word receives at most one increment per byte of the planes, so none can wrap below that bound.
 * More rows: KBBQ_E_ARG naming the limit -- cut them into several calls; they add into the same counts.
 * Refused on the arguments alone, before any HIP call (KBBQ_E_ARG, the function's name in kbbq_last_error()): a NULL ctx, plane,
 * d_len or d_counts1536; nreads < 0; a pitch that is not a positive multiple of 16; planes not 16-byte aligned; a qoffset
 * outside 0..255; the limit.
 * nreads == 0 returns KBBQ_OK and launches nothing.                                                                   */
#define KBBQ_CONFUSION_MAX_BASES 4294967295ull
int kbbq_flag_confusion_dev(kbbq_ctx* ctx, const uint8_t* d_qual, const uint8_t* d_truth, const uint8_t* d_kflags,
                            const uint32_t* d_len, int64_t nreads, int pitch, int qoffset, int64_t* d_counts1536);

/* ---- mate-pair rows: an optional device layout for paired reads of one length S --------------
 * One row per pair: [mate 1: S bytes][separator][mate 2: S bytes][padding to a multiple of 16];
 * separator and padding are 'N' (seq, cseq) / 0 (qual): uncounted bases.  For 2 x 150 bp the pitch
 * is 304 instead of 2 x 160: 5 % fewer bytes through HBM for the same bases.  K1 / K2 run on these
 * rows as on single reads (byte offset = stored cycle index; the separator gives mate 2's first
 * base "no previous base"); results are identical to the one-read-per-row path.  Preconditions
 * (the caller checks): reads alternate first / second in pair, both mates have length S = S2 / 2
 * and the same read group.  Data errors (quality > 42, alphabet) and rows the fast apply cannot
 * serve are reported through kbbq_ctx_status with ROW indices / as KBBQ_E_LUT: re-run on
 * one-read-per-row planes for the reference's exact error.
 * sidecar of a pair row: (2S + 1) | read group << 16.
 * kbbq_pack_pairs_dev: planes [2 * npairs, pitch] + sidecars -> pair planes [npairs, kbbq_pair_pitch(S2)]
 * (d_cseq / d_pcseq may be NULL); kbbq_unpack_pairs_dev: one pair plane (the K2 output) -> [2 * npairs, pitch].
 * kbbq_pair_lut_dev derives the pair-row apply LUT (kbbq_pair_lut_bytes) from the blob kbbq_solve_dev /
 * kbbq_build_lut produced (its flags must be 0: values fit int8 and stay in 0..255).          */
int    kbbq_pair_pitch(int S2);
size_t kbbq_pair_lut_bytes(int R, int Qt, int S2);
int    kbbq_pack_pairs_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                           const uint32_t* d_meta, int64_t npairs, int pitch, int S2,
                           uint8_t* d_pseq, uint8_t* d_pcseq, uint8_t* d_pqual, uint32_t* d_pmeta);
int    kbbq_unpack_pairs_dev(kbbq_ctx* ctx, const uint8_t* d_pplane, int64_t npairs, int S2, int pitch, uint8_t* d_plane);
int    kbbq_accumulate_pairs_dev(kbbq_ctx* ctx, const uint8_t* d_pseq, const uint8_t* d_pcseq, const uint8_t* d_pqual,
                                 const uint32_t* d_pmeta, int64_t npairs, int R, int S2, int minscore,
                                 int dinuc_minscore, int64_t* d_tables);
int    kbbq_pair_lut_dev(kbbq_ctx* ctx, const void* d_lut_blob, int R, int S2, int minscore, void* d_pair_lut);
/* the same for rows described by layout flags (below): KBBQ_ROWS_PAIRS [| KBBQ_ROWS_NIBBLES] [| KBBQ_ROWS_TWINS] */
int    kbbq_pair_lut_rows_dev(kbbq_ctx* ctx, const void* d_lut_blob, int R, int S2, int minscore, int flags, void* d_pair_lut);
int    kbbq_apply_pairs_dev(kbbq_ctx* ctx, const uint8_t* d_pseq, const uint8_t* d_pqual, const uint32_t* d_pmeta,
                            int64_t npairs, int R, int S2, int minscore, const void* d_lut_blob,
                            const void* d_pair_lut, uint8_t* d_pout);

/* ---- rows grouped by read group -----------------------------------------------------------
 * With many read groups each K1 workgroup (its LDS tables hold ONE group) used to scan every row and keep
 * its own, and K2's table-driven LUT outgrew the LDS.  If the caller orders the rows by read group
 * (stable: any order within a group gives the same counts) and passes d_seg[R + 1] -- group g owns rows
 * [d_seg[g], d_seg[g + 1]) -- every slice walks only its rows with all lanes busy and stages only its
 * group's LUT rows: any number of read groups runs at the single-group rate.  `pairs` selects mate-pair
 * rows (then pitch must be kbbq_pair_pitch(S2) and d_pair_lut comes from kbbq_pair_lut_dev; NULL otherwise).
 * The fast apply LUT must be range-safe (blob flags 0); rows it cannot serve are reported (KBBQ_E_LUT).  */
int    kbbq_accumulate_grouped_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                                   const uint32_t* d_meta, int64_t nrows, int pitch, int pairs, int R, int S2,
                                   int S_band, int S_min, int minscore, int dinuc_minscore, const int64_t* d_seg,
                                   int64_t* d_tables);      /* S_band, S_min as in kbbq_accumulate_band_dev (0 with pairs) */
int    kbbq_apply_grouped_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta,
                              int64_t nrows, int pitch, int pairs, int R, int S2, int minscore,
                              const void* d_lut_blob, const void* d_pair_lut, const int64_t* d_seg, uint8_t* d_out);

/* ---- layouts in one interface: flags, 4-bit sequence planes, the layout pass -----------------
 * KBBQ_ROWS_PAIRS   the rows are mate-pair rows (above; pitch = kbbq_pair_pitch(S2)).
 * KBBQ_ROWS_NIBBLES the seq / cseq planes hold one NIBBLE per base instead of one character: the nucleotide
 *                   code of compare_reads.py:199 (A0 T1 G2 C3; 4 = N, separator, padding), row stride pitch / 2,
 *                   8 bytes per 16-base chunk; word w (0, 1) of a chunk holds bases 8w..8w+3 in the low nibbles of
 *                   its bytes and bases 8w+4..8w+7 in the high nibbles.  Only batches whose seq AND cseq are
 *                   entirely ACGTN have such planes (kbbq_lay_out_dev reports KBBQ_E_LUT otherwise: keep byte
 *                   planes, which carry the reference's TypeError semantics); find_corrected_sites
 *                   (recalibrate.py:13-20) then compares codes.  K1 reads 2 B/base instead of 3, K2 2.5 instead of 3.
 * kbbq_accumulate_rows_dev / kbbq_apply_rows_dev: K1 / K2 on any combination (d_seg NULL: rows not grouped).
 * d_perm (apply, optional, with d_seg): row i of the batch is STORED as row d_perm[i] of d_out -- the rows go
 * straight back into the order they had before kbbq_group_rows_dev, no separate pass.
 * kbbq_meta_stats_dev: one pass over the sidecars (synchronises): h_stats8[0] shortest non-empty read, [1] longest
 * read, [2] largest read-group id, [3] violations of the mate-pair preconditions (0 = uniform first / second pairs
 * of one length and read group), [4] empty reads, [5] violations of the KBBQ_ROWS_TWINS preconditions (0 = single-end reads of one
 * length whose neighbours 2p / 2p+1 share a read group).
 * kbbq_group_rows_dev: stable counting sort of the rows (pairs != 0: of the PAIRS, by the first mate's sidecar)
 * by read group, R <= 256: d_perm[nrows] (row i of the grouped order is row d_perm[i]) and d_seg[R + 1];
 * d_work: kbbq_group_rows_work_bytes(nrows, R) bytes.  A sidecar with read group >= R -> KBBQ_E_RANGE (status).
 * kbbq_lay_out_dev: input-order rows [nreads, pitch] -> the destination layout in ONE pass (pair packing, gather by
 * d_perm (may be NULL), nibble packing fused): destination planes [nrows, dpitch] (seq / cseq: dpitch / 2 with
 * KBBQ_ROWS_NIBBLES), nrows = nreads / 2 and dpitch = kbbq_pair_pitch(S2) with KBBQ_ROWS_PAIRS, else nreads and pitch.  */
#define KBBQ_ROWS_PAIRS    1
#define KBBQ_ROWS_NIBBLES  2
/* KBBQ_ROWS_TWINS (with KBBQ_ROWS_PAIRS): the two reads of every row are BOTH first in pair -- single-end input of one
 * length packed two reads to a mate-pair row (same planes, same sidecar, same 5 % fewer bytes); the second half of a row
 * then counts into / looks up the forward cycle columns [0, S) like the first half instead of the mirrored ones
 * (compare_reads.py:304-306: no "/2" in the name).  Precondition (kbbq_meta_stats_dev h_stats8[5] == 0): no read is second
 * in pair, reads 2p and 2p+1 share their read group, all reads have one length (an odd count is fine: the last row's second
 * half is padding, kbbq_lay_out_dev writes (nreads + 1) / 2 rows).  kbbq_accumulate_rows_dev and
 * kbbq_pair_lut_rows_dev take the flag (the apply kernel reads it out of the LUT); kbbq_lay_out_dev packs such rows as any
 * other pair rows.  */
#define KBBQ_ROWS_TWINS    4
/* KBBQ_ROWS_ERRBIT (only with KBBQ_ROWS_NIBBLES | KBBQ_ROWS_PAIRS, with or without TWINS, on rows of 19 or 13 chunks -- 2 x 150
 * and 2 x 100 bp): in every nibble of the seq plane bits 0-2 are the code (0..4) and bit 3 is 1 exactly where the corrected
 * read's code differs from it (a corrected code 5, "an N that counts as an error", sets it like any other difference);
 * separator and padding are code 4 with bit 3 clear.  That bit is all the tally ever took from the corrected plane, so
 * kbbq_accumulate_rows_dev reads d_seq, d_qual and d_meta only -- d_cseq is not read and may be NULL (1.57 instead of 2.08
 * bytes per base) -- and kbbq_apply_rows_dev ignores the bit.  A nibble whose low three bits are 5..7 is a corrupt plane
 * (KBBQ_E_LUT on the status) with or without the flag; without the flag bit 3 set is one too, as before.
 * Written by kbbq_lay_out_dev (d_cseq required, d_lcseq may be NULL: no corrected plane is written) and by kbbq_fastq_fill_rows
 * (b required, cseq may be NULL), byte for byte alike.  Accepted by kbbq_accumulate_rows_dev, kbbq_apply_rows_dev,
 * kbbq_pair_lut_rows_dev (ignored), kbbq_accumulate_bands_dev / kbbq_apply_bands_dev (such a band is launched alone).  Every
 * other call that takes KBBQ_ROWS_* flags -- the k-mer calls on rows, kbbq_canonical_reads_rows_dev -- returns KBBQ_E_ARG
 * naming itself: it would read bit 3 as part of a code.  kbbq_unpack_nibbles_dev decodes bits 0-2 and so serves both kinds.  */
#define KBBQ_ROWS_ERRBIT   8
int    kbbq_accumulate_rows_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                                const uint32_t* d_meta, int64_t nrows, int pitch, int flags, int R, int S2, int S_band,
                                int S_min, int minscore, int dinuc_minscore, const int64_t* d_seg, int64_t* d_tables);
int    kbbq_apply_rows_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows,
                           int pitch, int flags, int R, int S2, int minscore, const void* d_lut_blob, const void* d_pair_lut,
                           const int64_t* d_seg, const int64_t* d_perm, uint8_t* d_out);
int    kbbq_meta_stats_dev(kbbq_ctx* ctx, const uint32_t* d_meta, int64_t nreads, int32_t* h_stats8);
/* ---- all length bands of a mixed-length input in one launch per kernel (BASELINE config 5) --------------------
 * The reference grows its count arrays as the reads get longer (recalibrate.py:81-101) and tallies / applies read by read;
 * the file path cuts a (length-sorted: SURVEY H2) input into bands of one row width each and used to launch K1 and K2 once
 * per band -- pipeline fill, table zeroing and flush paid per band.  kbbq_accumulate_bands_dev / kbbq_apply_bands_dev take
 * the whole list: bands the merged kernels serve (K1: every shape the table-driven kernel fits except the
 * chunk-position-major form of 2 x 150 bp mate-pair rows; K2: one-read-per-row 4-bit planes, one read group, the shapes the
 * short-lived kernel takes) run as ONE launch, every band on its share of the workgroups with its own pitch, LDS table
 * geometry (S_band, S_min as in kbbq_accumulate_band_dev) and pitch-narrowed LUT; the others are launched as
 * kbbq_accumulate_rows_dev / kbbq_apply_rows_dev (or kbbq_accumulate_band_dev / kbbq_apply_dev for flags == 0 without d_seg)
 * would launch them.  Results are those of the per-band calls (counts ADD into d_tables; every band's d_out gets its new
 * qualities); d_cseq is not read by apply, d_perm / d_out / d_pair_lut not by accumulate. */
typedef struct kbbq_band {
    const uint8_t* d_seq; const uint8_t* d_cseq; const uint8_t* d_qual; const uint32_t* d_meta;
    int64_t nrows; int32_t pitch; int32_t flags;           /* KBBQ_ROWS_* */
    int32_t S_band; int32_t S_min;                         /* longest / shortest read of the band (0: as kbbq_accumulate_band_dev) */
    const int64_t* d_seg; const int64_t* d_perm;           /* rows grouped by read group (may be NULL) */
    uint8_t* d_out; const void* d_pair_lut;                /* apply: output plane; mate-pair rows: kbbq_pair_lut_rows_dev's LUT */
} kbbq_band;
int    kbbq_accumulate_bands_dev(kbbq_ctx* ctx, const kbbq_band* bands, int nbands, int R, int S2, int minscore,
                                 int dinuc_minscore, int64_t* d_tables);
int    kbbq_apply_bands_dev(kbbq_ctx* ctx, const kbbq_band* bands, int nbands, int R, int S2, int minscore, const void* d_lut_blob);
size_t kbbq_group_rows_work_bytes(int64_t nrows, int R);
int    kbbq_group_rows_dev(kbbq_ctx* ctx, const uint32_t* d_meta, int64_t nrows, int pairs, int R, void* d_work,
                           int64_t* d_perm, int64_t* d_seg);
int    kbbq_lay_out_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_cseq, const uint8_t* d_qual,
                        const uint32_t* d_meta, int64_t nreads, int pitch, int flags, int S2, const int64_t* d_perm,
                        uint8_t* d_lseq, uint8_t* d_lcseq, uint8_t* d_lqual, uint32_t* d_lmeta);
int    kbbq_unpack_nibbles_dev(kbbq_ctx* ctx, const uint8_t* d_nib, int64_t nbases, uint8_t* d_chars);
/* d_dst[i] += d_src[i], i < n: count tables tallied apart (a length band, a layout tried first) into the file's */
int    kbbq_tables_add_dev(kbbq_ctx* ctx, int64_t* d_dst, const int64_t* d_src, size_t n);

/* ---- the exchange step of the sharded path without torch: RCCL allreduce of the count tables -------------
 * Reads shard across GPUs by contiguous record ranges, every rank tallies its shard (K1) and the ONLY exchange is the
 * sum of the int64 count-table buffers; marginals, meanq and the solve are then replicated and K2 is
 * local.  One process (or thread) per GPU, each with its own kbbq_ctx.  Rank 0 obtains a 128-byte id
 * (kbbq_comm_unique_id) and hands it to the other ranks by whatever channel the caller has (file, socket, MPI);
 * every rank then calls kbbq_comm_create with the same id -- collective, as ncclCommInitRank is.
 * kbbq_allreduce_tables: in place, enqueued on the context's stream (ordered between K1 and the solve, no host wait).
 * librccl is bound at the first call with dlopen (a copy already loaded by the process, else KBBQ_RCCL_LIB /
 * kbbq_comm_library(path), else the loader's librccl.so.1, else /opt/rocm/lib): libkbbq_hip.so itself does not link it.
 * The Python layer of this repository uses torch.distributed for the same step (kbbq/parallel.py); these entry points
 * are for C / C++ / other-language callers.  */
#define KBBQ_COMM_ID_BYTES 128
typedef struct kbbq_comm kbbq_comm;
int kbbq_comm_library(const char* path);
int kbbq_comm_unique_id(void* id128);
int kbbq_comm_create(kbbq_ctx* ctx, const void* id128, int nranks, int rank, kbbq_comm** out);
int kbbq_allreduce_tables(kbbq_comm* comm, int64_t* d_buf, size_t n);
int kbbq_comm_destroy(kbbq_comm* comm);

/* ---- host SAM / BAM reader (no GPU) ----------------------------------------------------------
 * Replaces, for the truth-set benchmark and the BAM-sourced tally, what the reference gets from
 * pysam.AlignmentFile / AlignedSegment (benchmark.py:57-74,102-143; gatk/bqsr.py:23-123): per alignment
 * the flag, contig, position, CIGAR, mate position, template length, sequence, qualities and the RG / OQ
 * tags, as arrays (the kernels take whole batches).  SAM text, gzip-compressed SAM or BAM (the reference's own input);
 * mapped, inflated where needed, indexed and parsed in parallel.
 * kbbq_sam_info: { alignments, CIGAR operations, longest SEQ, contigs seen, @RG lines, header lines }.
 * kbbq_sam_fields (any pointer may be NULL): flag; contig = index into the first-appearance list of RNAME;
 * pos / pnext 0-based; tlen; qlen = len(SEQ) (0 for '*'); ref_span = reference_end - reference_start;
 * clip = query_alignment_start | query_alignment_end << 16; cig_off / cig_n into kbbq_sam_cigar's array
 * (length << 4 | BAM op code, unknown letter = 15); rg = index of the RG:Z tag among the header's @RG IDs
 * (-1 no tag, -2 not in the header); has_qual_oq = len(QUAL) (0 for '*') | len(OQ:Z) << 16 (-1 << 16 when absent).
 * kbbq_sam_fill: plane rows [0, n) <- SEQ (0) / QUAL (1) / OQ (2) of alignments [first, first + n), zero padded.
 * kbbq_sam_text: 0 QNAME, 1 whole alignment line, 2 header line, 3 contig name, 4 @RG ID (not NUL-terminated).  */
typedef struct kbbq_sam kbbq_sam;
/* path: SAM text, gzip / bgzip-compressed SAM, or BAM (inflated with zlib, records rendered as SAM lines) */
int kbbq_sam_open(const char* path, kbbq_sam** out);
int kbbq_sam_close(kbbq_sam* f);
int kbbq_sam_info(const kbbq_sam* f, int64_t* info6);
int kbbq_sam_fields(const kbbq_sam* f, int32_t* flag, int32_t* contig, int64_t* pos, int64_t* pnext, int64_t* tlen,
                    int32_t* qlen, int32_t* ref_span, uint32_t* clip, uint32_t* cig_off, uint32_t* cig_n, int32_t* rg,
                    int32_t* has_qual_oq);
int kbbq_sam_cigar(const kbbq_sam* f, uint32_t* ops);
/* trim[i] = lo | hi << 16: query positions [lo, hi) of alignment i lie past its adaptor boundary (0: none) -- the reference's
 * bamread_adaptor_boundary + trim_bamread (gatk/bqsr.py:131-206) for every alignment of the file, by CIGAR walk. */
int kbbq_sam_adaptor_trim(const kbbq_sam* f, uint32_t* trim);
/* A whole regular file as bytes, inflated when it is gzip / bgzip (bgzip blocks side by side, gzip members chunk-wise on all host threads):
 * where kbbq/aln.py's FASTA / VCF / BED readers (the reference reads those through pysam: benchmark.py:9-55) take their text from.
 * *data stays valid until kbbq_text_close. */
typedef struct kbbq_text kbbq_text;
int kbbq_text_open(const char* path, kbbq_text** out, const uint8_t** data, size_t* n);
int kbbq_text_close(kbbq_text* t);
int kbbq_sam_fill(const kbbq_sam* f, int64_t first, int64_t n, int pitch, int which, uint8_t* plane);
int kbbq_sam_text(const kbbq_sam* f, int what, int64_t i, const char** p, int64_t* len);
/* kbbq_sam_render: alignments [first, first + n) as SAM lines ('\n'-terminated), each its own text with the QUAL field
 * replaced by row r of `qplane` (the field's own length; a '*' QUAL is kept) -- what applybqsr writes.  set_oq: append
 * "\tOQ:Z:<QUAL as read>" to a record without an OQ tag (an existing tag is kept).  out == NULL: *used = the bytes needed;
 * otherwise out holds cap bytes (KBBQ_E_ARG when they do not suffice) and *used = the bytes written.                     */
int kbbq_sam_render(const kbbq_sam* f, int64_t first, int64_t n, const uint8_t* qplane, int pitch, int set_oq,
                    uint8_t* out, size_t cap, size_t* used);


/* ---- host FASTQ ingest / egress (no GPU) ----------------------------------
 * Replaces, for this path, pysam.FastxFile iteration (recalibrate.py:56-57,141-142),
 * the name parsing of compare_reads.py:304-318 / recalibrate.py:59-64 and the print()
 * calls of recalibrate.py:153-156.  4-line records; name = header up to whitespace.
 * kbbq_fastq_scan(a, b|NULL, infer_rg, info[5]) validates in the reference's order and
 * returns info = { usable reads, longest read S, read groups R, error kind, error index }
 * with kinds 1 RG inference IndexError, 2 RG AssertionError, 3 name prefix
 * (AssertionError), 4 length mismatch (ValueError), 5 shorter than the running maximum
 * (IndexError; that read is still included so the device can check it first).
 * kbbq_fastq_fill packs reads [0, n) into the padded planes (multi-threaded);
 * kbbq_fastq_format renders "@name\nseq\n+\nqual\n" records with the new qualities.  */
typedef struct kbbq_fastq kbbq_fastq;
int         kbbq_fastq_open(const char* path, kbbq_fastq** out);
int         kbbq_fastq_close(kbbq_fastq* f);
/* multi-GPU ingest: rank 0 opens and scans the whole file, the other ranks index only their shard's byte range
 * [byte_lo, byte_hi) (record starts from kbbq_fastq_record_offset; byte_hi < 0: to the end; uncompressed files only,
 * kbbq_fastq_is_plain) and take the file-wide read-group names from rank 0 (count NUL-terminated strings). */
int         kbbq_fastq_open_range(const char* path, int64_t byte_lo, int64_t byte_hi, kbbq_fastq** out);
/* The first record start at or after `offset` (the file size when there is none; -1 on error): a rank of a multi-GPU
 * run cuts ITS byte range out of an uncompressed file with it, nobody indexes the whole file (kbbq/fastx.py). */
int64_t     kbbq_fastq_sync_offset(const char* path, int64_t offset);
/* skip_second != 0: never cut in front of a second-in-pair record (name field ends with "/2"): mates stay together */
int64_t     kbbq_fastq_sync_offset_ex(const char* path, int64_t offset, int skip_second);
int64_t     kbbq_fastq_record_offset(const kbbq_fastq* f, int64_t i);
int         kbbq_fastq_is_plain(const kbbq_fastq* f);
int         kbbq_fastq_set_rg_names(kbbq_fastq* f, const char* names, int count);
int64_t     kbbq_fastq_count(const kbbq_fastq* f);
int         kbbq_fastq_name(const kbbq_fastq* f, int64_t i, const char** name, int* len);
int         kbbq_fastq_rg_count(const kbbq_fastq* f);
const char* kbbq_fastq_rg_name(const kbbq_fastq* f, int i);
int         kbbq_fastq_scan(kbbq_fastq* a, const kbbq_fastq* b, int infer_rg, int64_t* info5);
/* ---- the same files read SEQUENTIALLY (csrc/fastq_stream.cpp): inputs that cannot be mapped or sought, inputs of any size ----
 * The reference walks its inputs read by read in constant memory (recalibrate.py:56-57 zip(FastxFile(A), FastxFile(B)),
 * :141-156 a second walk over A), so `-f <(zcat a.fq.gz) <(zcat b.fq.gz)` and files larger than memory work there.  A
 * kbbq_fastq_stream hands out SEGMENTS -- whole records, each an ordinary kbbq_fastq over memory of its own (scan / meta /
 * fill_rows / format work on it; close it with kbbq_fastq_close): the leading file about `max_bytes` per segment
 * (records = 0), the following file exactly the leader's number of records (records > 0; fewer only when it ends first: zip()
 * stops there).  *segment = NULL when the input has ended; *at_end = 1 when it ends behind this segment.  path: a regular
 * file, a named pipe / process substitution, "-" = standard input; gzip / bgzip bytes (a .fq.gz file of any size, a pipe that
 * carries them) are inflated as they are read, member after member, in constant memory -- as pysam.FastxFile reads them.
 * kbbq_fastq_stream_tee: every byte handed out is also appended to `fd` -- the spool a pipe's file A is kept in for pass 2.
 * kbbq_fastq_scan_next: kbbq_fastq_scan of one segment, with what the reference's walk carries from read to read handed
 * over by the caller: the read groups met so far (kbbq_fastq_set_rg_names first; new ones are appended, first-appearance
 * order over the whole input, recalibrate.py:59-64) and the longest read so far (recalibrate.py:89-101).                  */
typedef struct kbbq_fastq_stream kbbq_fastq_stream;
int         kbbq_fastq_stream_open(const char* path, kbbq_fastq_stream** out);
int         kbbq_fastq_stream_is_regular(const kbbq_fastq_stream* s);
int         kbbq_fastq_stream_tee(kbbq_fastq_stream* s, int fd);
int         kbbq_fastq_stream_next(kbbq_fastq_stream* s, size_t max_bytes, int64_t records, kbbq_fastq** segment, int* at_end);
int         kbbq_fastq_stream_prefetch(kbbq_fastq_stream* s, size_t bytes);   /* read ahead until `bytes` wait in the stream (another thread, while the leading file is read) */
int         kbbq_fastq_stream_close(kbbq_fastq_stream* s);
int         kbbq_fastq_scan_next(kbbq_fastq* a, const kbbq_fastq* b, int infer_rg, int64_t prior_longest, int64_t* info5);
/* kbbq_fastq_open of both files (b may be NULL) + kbbq_fastq_scan on the library's own threads; _begin returns at
 * once, _wait joins, hands over the readers and info5 and frees the job (call it exactly once).  File A's error is
 * reported before file B's.  Lets a Python caller set its device up while the files are being read. */
typedef struct kbbq_fastq_job kbbq_fastq_job;
int         kbbq_fastq_pair_begin(const char* path_a, const char* path_b, int infer_rg, kbbq_fastq_job** job);
int         kbbq_fastq_pair_wait(kbbq_fastq_job* job, kbbq_fastq** a, kbbq_fastq** b, int64_t* info5);
int         kbbq_fastq_lengths(const kbbq_fastq* f, int64_t first, int64_t n, uint32_t* out);   /* sequence lengths */
/* length bands of reads [first, first + n): maximal runs of reads of one length class (class = first entry of the
 * ascending classes[] >= the length); out[run] = {lo, hi, longest, shortest non-empty}; returns the number of runs,
 * or 1 run covering everything when there are more than max_runs */
int         kbbq_fastq_length_runs(const kbbq_fastq* f, int64_t first, int64_t n, const uint32_t* classes, int nclasses,
                                   int max_runs, int64_t* out);
int         kbbq_fastq_fill(const kbbq_fastq* a, const kbbq_fastq* b, int infer_rg, int64_t n, int pitch,
                            uint8_t* seq, uint8_t* cseq, uint8_t* qual, uint32_t* meta);
/* the same for reads [first, first + n) -> rows [0, n): one rank's shard; read-group ids are those of the scan */
int kbbq_fastq_fill_range(const kbbq_fastq* a, const kbbq_fastq* b, int infer_rg, int64_t first, int64_t n, int pitch,
                          uint8_t* seq, uint8_t* cseq, uint8_t* qual, uint32_t* meta);
/* ---- the packer writes the device layout itself (no kbbq_lay_out_dev pass, 2 B/base over PCIe instead of 3) ----
 * Replaces, like kbbq_fastq_fill_range, the pysam iteration + per-read arrays of recalibrate.py:56-57,89-101,141-148, but
 * hands the kernels the layout they are measured on: mate-pair rows / 4-bit sequence planes / rows gathered by
 * read-group segment (KBBQ_ROWS_* above), byte for byte what kbbq_lay_out_dev would make of kbbq_fastq_fill_range's rows.
 * kbbq_fastq_meta: the sidecar words of reads [first, first + n) (read-group ids of the scan) and the statistics of
 * kbbq_meta_stats_dev over them (stats8, same slots) -- what decides which layout the reads qualify for.
 * kbbq_group_rows_host: the stable counting sort of kbbq_group_rows_dev on the host (perm, seg).
 * kbbq_fastq_fill_rows: destination rows [row_lo, row_lo + nrows) of that band into plane rows 0 .. nrows - 1 (seq / cseq:
 * row stride pitch / 2 with KBBQ_ROWS_NIBBLES); KBBQ_ROWS_PAIRS: pitch = kbbq_pair_pitch(S2) (the argument is ignored) and
 * every read has length S2 / 2; perm (may be NULL): destination row r holds source row perm[r].  *foreign is set to 1 when
 * a seq / cseq letter outside ACGTN met the nibble packing: repeat the band without KBBQ_ROWS_NIBBLES (character planes
 * carry the reference's TypeError rule, compare_reads.py:224,292).
 * kbbq_fastq_format_rows: kbbq_fastq_format reading the new qualities out of the layout K2 wrote them in (mate-pair rows:
 * read first + i at row i / 2, byte offset (i & 1) * (S2 / 2 + 1)) -- recalibrate.py:153-156 without an unpack pass.  */
int         kbbq_fastq_meta(const kbbq_fastq* a, int infer_rg, int64_t first, int64_t n, uint32_t* meta, int32_t* stats8);
int         kbbq_group_rows_host(const uint32_t* meta, int64_t nrows, int pairs, int R, int64_t* perm, int64_t* seg);
int         kbbq_fastq_fill_rows(const kbbq_fastq* a, const kbbq_fastq* b, int64_t first, int64_t n, const uint32_t* meta,
                                 int flags, int S2, int pitch, const int64_t* perm, int64_t row_lo, int64_t nrows,
                                 uint8_t* seq, uint8_t* cseq, uint8_t* qual, uint32_t* dmeta, int* foreign);
int64_t     kbbq_fastq_format_rows(const kbbq_fastq* a, int64_t first, int64_t n, int flags, int S2, int pitch,
                                   const uint8_t* newqual, char* out, int64_t cap);
/* benchmark.py:102-124: idx[i] = the alignment whose QNAME + "/1"|"/2" equals the name of FASTQ read i up to its
 * first '_' (the last such alignment), -1 if none.                                                   */
int         kbbq_sam_match_fastq(const kbbq_sam* f, const kbbq_fastq* fq, int64_t* idx);
int64_t     kbbq_fastq_format(const kbbq_fastq* a, int64_t first, int64_t n, int pitch,
                              const uint8_t* newqual, char* out, int64_t cap);

/* ---- synthetic reads (bench / tests) -----------------------
 * Device twin of the generator documented in oracle/kbbq_oracle.c.          */
int kbbq_synth_dev(kbbq_ctx* ctx, uint8_t* d_seq, uint8_t* d_cseq, uint8_t* d_qual,
                   uint32_t* d_meta, int64_t first_read, int64_t nreads, int64_t total_reads,
                   int pitch, uint64_t seed, int len_lo, int len_hi, int nrg,
                   int qlo, int qhi, const uint32_t* thr43);

/* ---- timing of the most recent kernels (bench.py roofline) -------------
 * When enabled, every K1 / K2 launch is bracketed by HIP events on the launch
 * stream; kbbq_ctx_kernel_ms returns the accumulated milliseconds and launch
 * counts since the last reset (synchronises).  which: 0 = K1, 1 = K2.       */
int kbbq_ctx_timing(kbbq_ctx* ctx, int enable);
int kbbq_ctx_kernel_ms(kbbq_ctx* ctx, int which, double* total_ms, int64_t* launches, int reset);

/* ---- k-mer counting and single-substitution correction (kbbq correct; csrc/kbbq_kmer.h) ---------------------------------------
 * The step the reference leaves to an external corrector (docs/tutorials/recalibration.rst, "Correcting Reads"): its output is
 * the second file of `kbbq recalibrate -f`.  Rows are a seq plane and meta words as above (only the length bits are read).
 * A base is A C G T (uppercase); any other byte, and every byte at or beyond the read's length, is a break.  A k-mer is a
 * window of k (8..32) bases without a break, keyed by its canonical 2k-bit code (the smaller of forward and reverse complement,
 * first base in the high bits).
 * Table: open addressing, `slots` a power of two, uint64 keys (all ones = empty) and uint32 counts, kbbq_kmer_table_bytes(slots)
 * bytes of device memory.  kbbq_kmer_table_info hands out the device arrays (keys[slots], counts[slots]) and the geometry.
 * kbbq_kmer_count_dev ADDS every k-mer of the rows to the table (slabs and batches compose); counts are exact.  An insert that
 * finds no free slot within a bounded probe sequence sets a status word: kbbq_ctx_status then returns KBBQ_E_FULL (read index
 * -1), and the table's content is not a valid count -- nothing is dropped silently.
 * kbbq_kmer_histogram_dev writes d_hist[257] (uint64): d_hist[c] = distinct k-mers with count c (1..255), d_hist[256] = those
 * with count >= 256, d_hist[0] = 0.  The caller picks the solid threshold from it (kbbq/kmer.py solid_threshold).
 * kbbq_kmer_correct_dev: a k-mer is solid when its count is >= min_count.  Base i is trusted when a solid k-mer covers it or
 * none covers it; an untrusted A/C/G/T base becomes the other base b whose substitution makes the most covering k-mers solid,
 * when that number is >= 1 and strictly larger than for the other two; every base is judged against the read as given.  d_out
 * (16-byte aligned, the input's layout) receives the corrected plane, breaks and padding as read; d_changed (may be NULL) the
 * number of changed bases per read.
 * N rule (kbbq correct --fix-n): kbbq_kmer_correct_ex_dev / kbbq_kmer_correct_ex / kbbq_kmer_correct_rows_ex_dev are the calls
 * without _ex plus `int opts`, a word of KBBQ_KMER_* bits (not the KBBQ_ROWS_* flags); opts = 0 IS the call without _ex, an
 * unknown bit returns KBBQ_E_ARG before anything is launched.  With KBBQ_KMER_FIX_N an 'N' at base i of a read (the character
 * 'N' alone; lower case and other letters stay breaks and stay as read) is handled as follows.  Its candidate windows are the
 * windows [s, s + k) with s <= i < s + k that lie inside the read and hold no other base outside A/C/G/T.  For each letter x of
 * A C G T, count the candidate windows whose canonical k-mer, with x written at i and every other base as read, has a count
 * >= min_count.  The N takes the letter with the strictly largest count if that count is >= 1; on a tie, or when no letter makes
 * a solid k-mer, it stays N.  Everything is judged against the read as given: a fixed N validates no window for its neighbours,
 * an untrusted A/C/G/T base beside an N is decided exactly as without the option (the N is a break for it), and the result does
 * not depend on thread order.  A fixed N is a changed base in d_changed.  Counting, the prefilter, the histogram and the
 * threshold know nothing of the option: an N is a break for them and the table is the same table.
 * kbbq_kmer_flag_dev: the decision of kbbq_kmer_correct_dev as a flag plane, for callers that want to know WHICH bases the solid
 * k-mers contradict and not what they become (kbbq bqsr --kmers: the errors of a recalibration tally).  Same arguments and
 * refusals (pitch a multiple of 16, min_count >= 1, NULL table / planes, nreads == 0 does nothing); d_flags (16-byte aligned,
 * [nreads, pitch]) receives 1 at every base where kbbq_kmer_correct_dev would write a byte different from d_seq's and 0
 * everywhere else -- breaks (N included: there is no N rule here), trusted bases, ties, padding up to pitch.  Every byte of every
 * row is written: the plane needs no clearing.  d_changed (may be NULL) as above.  The plane is, bit for bit, the one plane of
 * flags kbbq_accumulate_aligned_dev and kbbq_canonical_reads_rows_dev(d_skip = NULL) read: bit 0 error, bit 1 (skip) set only
 * by kbbq_kmer_flag_ex_dev with KBBQ_KMER_FLAG_UNRESOLVED.
 * kbbq_kmer_flag_ex_dev: kbbq_kmer_flag_dev plus `d_unresolved` and `int opts`, a word of KBBQ_KMER_* bits; opts = 0 with
 * d_unresolved = NULL IS kbbq_kmer_flag_dev.  An unknown bit, or KBBQ_KMER_FIX_N (the flag form has no N rule), returns
 * KBBQ_E_ARG before anything is launched.  The rule above has three outcomes for an A/C/G/T base inside the read: TRUSTED (a solid
 * k-mer covers it, or no k-mer window covers it at all), ERROR (untrusted, and one substitution makes strictly the most covering
 * k-mers solid, >= 1) and UNRESOLVED (untrusted -- at least one window covers it, none is solid -- and no substitution wins: a
 * tie, or none makes a solid k-mer).  An unresolved base is one the k-mers contradict without naming its replacement: two errors
 * within k bases of each other, a region too thinly covered to have solid k-mers, contamination.  With
 * KBBQ_KMER_FLAG_UNRESOLVED the byte of an unresolved base is 2 (the tally's skip bit: the base then counts neither as an error
 * nor as an observation); errors stay 1, trusted bases, breaks (N included) and padding stay 0, no byte is 3 and every byte of
 * every row is still written.  The decision does not depend on thread order.  d_changed keeps its meaning (bytes set to 1);
 * d_unresolved (uint32 per read, may be NULL) receives the number of bytes set to 2 in the read -- all zeros with opts = 0.
 * Passes (kbbq correct --passes P): kbbq_kmer_correct_passes_dev / kbbq_kmer_correct_passes / kbbq_kmer_correct_rows_passes_dev /
 * kbbq_kmer_flag_passes_dev are kbbq_kmer_correct_ex_dev / kbbq_kmer_correct_ex / kbbq_kmer_correct_rows_ex_dev /
 * kbbq_kmer_flag_ex_dev plus `int passes` (1..8), with every refusal of those calls; passes outside 1..8 returns KBBQ_E_ARG before
 * anything is launched, and passes = 1 IS the call without it (the same kernel).  Let C(row) be the rule above on one row --
 * the substitution rule, and with KBBQ_KMER_FIX_N the N rule -- against the table at min_count.  The table, and so every count,
 * comes from the reads as read: nothing is recounted between passes.  r_0 is the row as read and r_p = C(r_(p-1)): within a pass
 * every base is judged against r_(p-1) (no cascade inside a pass), an N fixed in pass p is an ordinary base from pass p + 1 on,
 * an N that stayed N may be fixed by a later pass once its windows have become solid, and the separator of a row of two reads
 * is never an N.  A pass that changes nothing in a row ends that row, later passes would repeat it.  The result is r_P and does not
 * depend on thread order.  Corrected form: d_out receives r_P, breaks and padding as read; d_changed the number of bases inside
 * the read where r_P differs from r_0 (not the sum of the passes' changes: a base changed and changed back counts nothing).
 * Flag form: 1 where r_P differs from r_0; with KBBQ_KMER_FLAG_UNRESOLVED 2 where the base is unchanged (r_P == r_0) and was
 * unresolved in the last evaluation of its row -- pass P, or the pass that found the fixed point; 0 elsewhere.  No byte is 3 and
 * every byte of every row is written; d_changed counts the 1s and d_unresolved the 2s.  A row is carried through its passes in
 * LDS: a pitch whose rows do not fit there returns KBBQ_E_ARG naming the bytes (8 words per 16 bases, where one pass needs 3).
 * kbbq_kmer_count / kbbq_kmer_correct: the same from host buffers, slab by slab through page-locked staging (KBBQ_STAGE_MB);
 * `changed` (host, may be NULL) receives the per-read counts.  The kernel launches are not timed by kbbq_ctx_timing.
 * Ranks (kbbq/kmer.py count_kmers_ranks): every rank counts its reads into a local table, sends each key to its owner and merges
 * what it receives into the table of the keys it owns.  kbbq_kmer_owner(key, W) = (uint32)(((mix(key ^ 0x9E3779B97F4A7C15) >>
 * 32) * W) >> 32), mix being the table's slot hash; the home slot uses the low bits of mix(key), the owner the high bits of
 * another mix, so the keys of one owner spread over every home slot of its table.  kbbq_kmer_table_clear_dev empties a table.
 * kbbq_kmer_select_sizes_dev (synchronous) writes h_sizes[b] = occupied slots with count >= min_count whose owner among
 * `nbuckets` (1..1024) is b; nbuckets = 1 counts them all.  kbbq_kmer_select_dev (synchronous) writes them: bucket b's keys and
 * counts to d_keys / d_counts [h_offsets[b], h_offsets[b] + h_sizes[b]), any order inside a bucket -- with h_offsets the
 * exclusive scan of h_sizes, one dense buffer in bucket order.  kbbq_kmer_merge_dev ADDS n (key, count) pairs (device arrays)
 * to a table with the probing of kbbq_kmer_count_dev; a pair that finds no free slot makes kbbq_ctx_status return KBBQ_E_FULL
 * as a count does.                                                                                                         */
typedef struct kbbq_kmer_table kbbq_kmer_table;
size_t kbbq_kmer_table_bytes(int64_t slots);
int kbbq_kmer_table_create_dev(kbbq_ctx* ctx, int k, int64_t slots, kbbq_kmer_table** out);
int kbbq_kmer_table_free_dev(kbbq_ctx* ctx, kbbq_kmer_table* table);
int kbbq_kmer_table_info(const kbbq_kmer_table* table, int* k, int64_t* slots, void** d_keys, void** d_counts);
int kbbq_kmer_count_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nreads,
                        int pitch);
int kbbq_kmer_histogram_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, uint64_t* d_hist);
int kbbq_kmer_correct_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                          int64_t nreads, int pitch, int min_count, uint8_t* d_out, uint32_t* d_changed);
int kbbq_kmer_flag_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                       int64_t nreads, int pitch, int min_count, uint8_t* d_flags, uint32_t* d_changed);
int kbbq_kmer_count(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint8_t* seq, const uint32_t* meta, int64_t nreads, int pitch);
int kbbq_kmer_correct(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* seq, const uint32_t* meta, int64_t nreads,
                      int pitch, int min_count, uint8_t* out, uint32_t* changed);
#define KBBQ_KMER_FIX_N 1
#define KBBQ_KMER_FLAG_UNRESOLVED 2
int kbbq_kmer_flag_ex_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                          int64_t nreads, int pitch, int min_count, uint8_t* d_flags, uint32_t* d_changed,
                          uint32_t* d_unresolved, int opts);
int kbbq_kmer_correct_ex_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                             int64_t nreads, int pitch, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts);
int kbbq_kmer_correct_ex(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* seq, const uint32_t* meta, int64_t nreads,
                         int pitch, int min_count, uint8_t* out, uint32_t* changed, int opts);
int kbbq_kmer_correct_passes_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                                 int64_t nreads, int pitch, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts, int passes);
int kbbq_kmer_correct_passes(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* seq, const uint32_t* meta, int64_t nreads,
                             int pitch, int min_count, uint8_t* out, uint32_t* changed, int opts, int passes);
int kbbq_kmer_flag_passes_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                              int64_t nreads, int pitch, int min_count, uint8_t* d_flags, uint32_t* d_changed,
                              uint32_t* d_unresolved, int opts, int passes);
int kbbq_kmer_table_clear_dev(kbbq_ctx* ctx, kbbq_kmer_table* table);
int kbbq_kmer_select_sizes_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, int nbuckets, uint32_t min_count, int64_t* h_sizes);
int kbbq_kmer_select_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, int nbuckets, uint32_t min_count, const int64_t* h_offsets,
                         uint64_t* d_keys, uint32_t* d_counts);
int kbbq_kmer_merge_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint64_t* d_keys, const uint32_t* d_counts, int64_t n);
uint32_t kbbq_kmer_owner(uint64_t key, int nbuckets);

/* ---- k-mer sets (kbbq count, --kmers-from; csrc/kbbq_kmer_set.h, kbbq/kmerset.py) -----------------------------------------------
 * A k-mer set is the (canonical key, count) pairs with count >= keep of a finished count, ascending by key as UNSIGNED 64-bit
 * words (k = 32 keys use bit 63), in a file kbbq/kmerset.py describes byte by byte.
 * kbbq_kmer_sort_pairs_dev sorts n pairs (device arrays, as kbbq_kmer_select_dev writes them) by unsigned key into d_keys_out /
 * d_counts_out, buffers of their own (KBBQ_E_ARG when an output is its input); only the 2k low key bits are looked at, keys are
 * expected to be distinct, and the result is then the same permutation whatever the thread order.  d_temp: at least
 * kbbq_kmer_sort_pairs_bytes(n) bytes of device memory (KBBQ_E_ARG naming both numbers otherwise).  Asynchronous on the
 * context's stream; n == 0 does nothing.
 * kbbq_kmer_check_pairs_dev (synchronous) judges one slab of n pairs, `first` being the global index of its pair 0: pair i must
 * have keys[i] > keys[i - 1] (the slab's pair 0 against prev_key when have_prev is not 0: the last key of the slab before),
 * keys[i] < 4^k, keys[i] <= the reverse complement of keys[i] (it is canonical) and counts[i] >= keep.  *bad_index receives
 * the lowest global index of a pair that breaks a rule, or -1, and *bad_reason the first rule it breaks in the order above
 * (KBBQ_KMER_PAIR_*; 0 when none does).  h_sums[0] += the sum of the keys and h_sums[1] += the sum of the counts, both modulo
 * 2^64, so the sums of a file's slabs add up in the caller's two words.  An offender is an answer, not an error: the return is
 * KBBQ_OK.  n == 0 does nothing.                                                                                               */
#define KBBQ_KMER_PAIR_ORDER      1   /* keys[i] <= the key before it (unsorted, or a duplicate)  */
#define KBBQ_KMER_PAIR_RANGE      2   /* keys[i] >= 4^k                                           */
#define KBBQ_KMER_PAIR_CANONICAL  3   /* keys[i] > its reverse complement                         */
#define KBBQ_KMER_PAIR_COUNT      4   /* counts[i] < keep                                         */
int kbbq_kmer_sort_pairs_bytes(kbbq_ctx* ctx, int64_t n, size_t* bytes);
int kbbq_kmer_sort_pairs_dev(kbbq_ctx* ctx, int k, const uint64_t* d_keys_in, const uint32_t* d_counts_in, uint64_t* d_keys_out,
                             uint32_t* d_counts_out, int64_t n, void* d_temp, size_t temp_bytes);
int kbbq_kmer_check_pairs_dev(kbbq_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, int64_t n, int k, uint32_t keep,
                              int64_t first, int have_prev, uint64_t prev_key, uint64_t* h_sums, int64_t* bad_index, int* bad_reason);

/* ---- prefilter: k-mers seen once stay out of the table (kbbq correct --prefilter; csrc/kbbq_kmer.h) ---------------------------
 * Nothing after the count looks at a k-mer seen once (the threshold starts at 2), and most distinct k-mers of real reads are
 * such.  A k-mer filter is two device arrays of `words` (a power of two) uint64 words, `seen` and `twice`, zero when created;
 * kbbq_kmer_filter_bytes(words) = 16 * words.  A canonical key has one word index and one mask of up to 4 bits, the same in
 * both arrays:
 *     h    = mix(key ^ 0xD6E8FEB86659FD93)        mix: the table's slot hash; a salt of its own (not the owner's)
 *     word = (h >> 24) & (words - 1)
 *     mask = OR over j = 0..3 of  1 << ((h >> 6 j) & 63)
 * Pass 1, kbbq_kmer_prefilter_dev, for every k-mer window of the rows (the windows kbbq_kmer_count_dev counts): OR mask into
 * seen[word]; if the value before held every bit of mask (the key, or a false positive, came before), OR mask into twice[word],
 * and where that OR set a new bit add one to the filter's `admitted` counter.  Both tests read the value one atomic returned
 * (or a load that already showed the whole mask: bits are only ever set), so of all occurrences of a key at most one finds its
 * mask incomplete: EVERY k-mer that occurs twice or more ends up in `twice`, whatever the thread order -- no false negatives.
 * `seen` after the pass is the OR of the masks of all distinct keys and does not depend on order; `twice` and `admitted` do
 * (which once-seen keys slip in as false positives varies).  `admitted` can undercount the keys in `twice` by those whose mask
 * other keys had completed there.  Passes over several row sets compose, as counting does.
 * Pass 2, kbbq_kmer_count_filtered_dev: kbbq_kmer_count_dev for the windows whose mask is wholly in twice[word]; any other
 * window is skipped.  Run after pass 1 has seen ALL rows, the table holds every k-mer of count >= 2 with its exact count,
 * some k-mers with exact count 1 (false positives) and nothing else: the histogram from c = 2 up, the threshold, the solid set
 * and kbbq_kmer_correct_dev's output at min_count >= 2 equal the unfiltered ones bit for bit.  h[1] counts the admitted
 * singletons only, so min_count = 1 has no meaning with a filtered table.  A table that fills reports KBBQ_E_FULL as above.
 * kbbq_kmer_filter_admitted is synchronous.  kbbq_kmer_filter_release_seen_dev (synchronous) frees `seen` once pass 1 is
 * over -- before the table is allocated, sized from `admitted` -- after which kbbq_kmer_filter_info returns NULL for it and
 * the filter takes no further pass 1 or clear.  kbbq_kmer_filter_clear_dev zeroes both arrays and the counter.
 * kbbq_kmer_prefilter / kbbq_kmer_count_filtered: the same from host buffers, each one more pass over the page-locked slabs
 * of kbbq_kmer_count.                                                                                                       */
typedef struct kbbq_kmer_filter kbbq_kmer_filter;
size_t kbbq_kmer_filter_bytes(int64_t words);
int kbbq_kmer_filter_create_dev(kbbq_ctx* ctx, int64_t words, kbbq_kmer_filter** out);
int kbbq_kmer_filter_free_dev(kbbq_ctx* ctx, kbbq_kmer_filter* filter);
int kbbq_kmer_filter_clear_dev(kbbq_ctx* ctx, kbbq_kmer_filter* filter);
int kbbq_kmer_filter_info(const kbbq_kmer_filter* filter, int64_t* words, void** d_seen, void** d_twice);
int kbbq_kmer_filter_admitted(kbbq_ctx* ctx, const kbbq_kmer_filter* filter, int64_t* admitted);
int kbbq_kmer_filter_release_seen_dev(kbbq_ctx* ctx, kbbq_kmer_filter* filter);
int kbbq_kmer_prefilter_dev(kbbq_ctx* ctx, kbbq_kmer_filter* filter, int k, const uint8_t* d_seq, const uint32_t* d_meta,
                            int64_t nreads, int pitch);
int kbbq_kmer_count_filtered_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const kbbq_kmer_filter* filter, const uint8_t* d_seq,
                                 const uint32_t* d_meta, int64_t nreads, int pitch);
int kbbq_kmer_prefilter(kbbq_ctx* ctx, kbbq_kmer_filter* filter, int k, const uint8_t* seq, const uint32_t* meta, int64_t nreads,
                        int pitch);
int kbbq_kmer_count_filtered(kbbq_ctx* ctx, kbbq_kmer_table* table, const kbbq_kmer_filter* filter, const uint8_t* seq,
                             const uint32_t* meta, int64_t nreads, int pitch);

/* ---- the k-mer calls on resident rows (kbbq recalibrate -c; csrc/kbbq_kmer.h "Row readers") ----------------------------------
 * The recalibrate file path keeps its reads on the device in the layouts of kbbq_accumulate_rows_dev: mate-pair or twin rows,
 * 4-bit sequence planes, rows grouped by read group.  These four are the calls above on such rows, `flags` the KBBQ_ROWS_* of
 * that call, so that reads are counted and corrected where they lie and K1 takes the corrected plane as its d_cseq.
 * KBBQ_ROWS_NIBBLES: d_seq (and d_out) are 4-bit planes -- row stride pitch / 2, 8 bytes per 16-base chunk, 8-byte aligned,
 * nibble order and codes (A0 T1 G2 C3, 4 = N / separator / padding) as documented above.  A code >= 4 is a break, and so is every
 * position at or beyond the row's length (the sidecar's low 16 bits).  The k-mer code stays the table's own (A0 C1 G2 T3,
 * canonical = the smaller of forward and reverse complement): keys, counts, the histogram and the filter words are those the
 * character calls produce for the same bases, and one table may be counted from rows of both kinds.  d_out receives the
 * corrected plane in the same 4-bit layout, breaks and padding as read.
 * KBBQ_ROWS_PAIRS / KBBQ_ROWS_TWINS need nothing of their own: a row's sidecar length is 2S + 1 and the separator is a break, so
 * no window spans two reads.  The flags are checked as kbbq_accumulate_rows_dev checks them (TWINS only with PAIRS) and pitch
 * must be a multiple of 16, which every kbbq_pair_pitch is; d_changed is per ROW (a mate-pair row counts both mates).
 * Without KBBQ_ROWS_NIBBLES the calls ARE the character calls above on the same rows.  Grouping by read group only orders the
 * rows: d_seg / d_perm are not needed here.
 * kbbq_kmer_correct_rows_ex_dev: kbbq_kmer_correct_rows_dev plus `opts` (KBBQ_KMER_FIX_N, above; `flags` keeps its meaning and its
 * refusals).  On a 4-bit plane an N is code 4 inside the row's length, and a fixed one is stored as its letter's plane code.
 * With KBBQ_ROWS_PAIRS the base at (length - 1) / 2 of a row is the separator of its two reads (an 'N' / code 4 too): it is
 * never fixed, and since every window across it holds that break no N takes a letter from the other read.  The padding half
 * of a twin row of one read is Ns beside Ns and stays as it is.
 * kbbq_kmer_correct_rows_skip_dev (kbbq recalibrate -c --skip-unresolved): kbbq_kmer_correct_rows_passes_dev -- the same flags,
 * opts (0 or KBBQ_KMER_FIX_N), passes (1..8), refusals and LDS limit, and bit for bit the same d_out and d_changed -- plus the
 * rule's third outcome as a second QUALITY plane.  d_qual is the rows' quality plane as read and d_tally_qual the tally plane,
 * both [nrows, pitch] characters (also beside a 4-bit sequence plane, whose row stride is pitch / 2) and 16-byte aligned.
 * d_tally_qual receives d_qual with byte 0 at every unresolved base: an untrusted A/C/G/T base no substitution wins, with
 * passes > 1 a base that ends as it was read and that the last evaluation of its row left unresolved (the 2s of the flag form).
 * Every byte of every row is written, separator and padding as read (they are breaks, never unresolved); d_qual is not
 * written.  kbbq_accumulate_rows_dev sends a base whose quality byte is below 33 + minscore to its trash row and looks at the
 * base's own byte alone for that, so a tally with d_tally_qual in the place of d_qual leaves exactly the unresolved bases out,
 * as an error and as an observation, and changes nothing for their neighbours.  d_unresolved (per row, may be NULL) receives
 * their number.  KBBQ_E_ARG before anything is launched: NULL d_qual or d_tally_qual, d_tally_qual == d_qual, a plane that is
 * not 16-byte aligned, KBBQ_KMER_FLAG_UNRESOLVED (the flag form's bit) or an unknown bit in opts.  nrows == 0 does nothing. */
int kbbq_kmer_count_rows_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                             int pitch, int flags);
int kbbq_kmer_prefilter_rows_dev(kbbq_ctx* ctx, kbbq_kmer_filter* filter, int k, const uint8_t* d_seq, const uint32_t* d_meta,
                                 int64_t nrows, int pitch, int flags);
int kbbq_kmer_count_filtered_rows_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const kbbq_kmer_filter* filter, const uint8_t* d_seq,
                                      const uint32_t* d_meta, int64_t nrows, int pitch, int flags);
int kbbq_kmer_correct_rows_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                               int64_t nrows, int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed);
int kbbq_kmer_correct_rows_ex_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                                  int64_t nrows, int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts);
/* ... plus `passes` (Passes, above): every layout, the N rule included */
int kbbq_kmer_correct_rows_passes_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                                      int64_t nrows, int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts,
                                      int passes);
int kbbq_kmer_correct_rows_skip_dev(kbbq_ctx* ctx, const kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta,
                                    int64_t nrows, int pitch, int flags, int min_count, uint8_t* d_out, uint32_t* d_changed, int opts,
                                    int passes, const uint8_t* d_qual, uint8_t* d_tally_qual, uint32_t* d_unresolved);

/* ---- partitions: one partition of the k-mers at a time (kbbq correct --partitions; csrc/kbbq_kmer.h "partitions") ------------
 * part(key, P) = kbbq_kmer_owner(key, P), the split the ranks use.  Each call below is its sibling without `_part` -- the same
 * arguments, refusals, table, probing and KBBQ_E_FULL -- for the windows whose canonical key has part(key, parts) == part, and
 * for no other window: the rows are read and every window is hashed, but only partition `part` is inserted (the filtered
 * forms test the partition before they read the filter).  Counting ADDS, and every key lies in exactly one partition: calling
 * all `parts` partitions into ONE table equals one kbbq_kmer_count_dev of the same rows, and calling partition p alone into an
 * empty table leaves exactly the keys of partition p there, each with its count over those rows -- so P rounds over all rows,
 * through a table 1 / P the size that is cleared between them (kbbq_kmer_table_clear_dev), see every key's global count once
 * (kbbq/kmer.py count_partitioned: the histograms of the rounds add up, kbbq_kmer_select_dev keeps the pairs that can be
 * solid, kbbq_kmer_merge_dev builds the table the correction reads from them).
 * parts must be in 1..1024 and part in 0..parts-1: anything else returns KBBQ_E_ARG naming the call, on the two numbers alone
 * and before any other argument is looked at; then come the sibling's own refusals.  parts == 1 IS the sibling: the same
 * kernel is launched.                                                                                                       */
int kbbq_kmer_count_part_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nreads,
                             int pitch, int parts, int part);
int kbbq_kmer_count_filtered_part_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const kbbq_kmer_filter* filter, const uint8_t* d_seq,
                                      const uint32_t* d_meta, int64_t nreads, int pitch, int parts, int part);
int kbbq_kmer_count_part(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint8_t* seq, const uint32_t* meta, int64_t nreads, int pitch,
                         int parts, int part);
int kbbq_kmer_count_filtered_part(kbbq_ctx* ctx, kbbq_kmer_table* table, const kbbq_kmer_filter* filter, const uint8_t* seq,
                                  const uint32_t* meta, int64_t nreads, int pitch, int parts, int part);
int kbbq_kmer_count_rows_part_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows,
                                  int pitch, int flags, int parts, int part);
int kbbq_kmer_count_filtered_rows_part_dev(kbbq_ctx* ctx, kbbq_kmer_table* table, const kbbq_kmer_filter* filter,
                                           const uint8_t* d_seq, const uint32_t* d_meta, int64_t nrows, int pitch, int flags, int parts,
                                           int part);

/* ---- quality gate: count only k-mers of bases with quality >= Q (kbbq correct --kmer-min-qual; csrc/kbbq_kmer.h km_gate) ------
 * THE RULE.  A base of a row is countable when it is A/C/G/T (as for every count call) and its quality byte in d_qual is
 * >= qual_byte_min; a window is counted iff all k of its bases are countable.  The call writes d_out, a copy of d_seq in the
 * same layout with 'N' (KBBQ_ROWS_NIBBLES: code 4) wherever the quality byte is < qual_byte_min and every other byte as read;
 * every byte of every row is written, padding and separator included.  An 'N' is a break to every count call, so
 * kbbq_kmer_prefilter*, kbbq_kmer_count*, kbbq_kmer_count_filtered* and their _part forms on d_out (with the same d_meta, pitch
 * and flags) see exactly the counted windows: counting d_out with any existing count call yields exactly *d_windows insertions.
 * Nothing after the count knows the gate: the correct / flag calls take d_seq as read.
 * d_qual is the rows' quality plane, [nrows, pitch] characters (also beside a 4-bit sequence plane, whose row stride is
 * pitch / 2) at the base's own row and column, 16-byte aligned.  qual_byte_min is a BYTE value: Q + 33 for character qualities,
 * Q + 0 for a plane of raw Phred values.  *d_windows (a device word, may be NULL: no count) is ADDED to, not set: the caller
 * zeroes it, so the bands of one input sum into one word.  d_seq and d_qual are not written.
 * flags are the KBBQ_ROWS_* of the calls above, checked as there; 0 is character rows, one read a row.  KBBQ_E_ARG naming the
 * call before anything is launched: a NULL plane or meta with nrows > 0, d_out == d_seq, a plane that is not aligned (4-bit
 * planes 8 bytes, character and quality planes 16), k outside 8..32, qual_byte_min outside 1..255, a pitch whose rows do not
 * fit the LDS.  nrows == 0 does nothing.  There is no host-buffer form. */
int kbbq_kmer_gate_rows_dev(kbbq_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint32_t* d_meta, int64_t nrows,
                            int pitch, int flags, int k, int qual_byte_min, uint8_t* d_out, uint64_t* d_windows);

/* ---- BGZF output: deflate on the GPU (--bgzf; csrc/kbbq_bgzf.h, kbbq/_bgzf.py) ------------------------------------------------
 * THE FORMAT.  n bytes of text are cut at multiples of block_bytes (1..KBBQ_BGZF_BLOCK_MAX; the last block is the remainder) and
 * every piece becomes one BGZF block, a complete gzip member: 1f 8b 08 04 00 00 00 00 00 ff 06 00 'B' 'C' 02 00, BSIZE - 1 as a
 * little-endian u16 (18 bytes), a raw deflate payload, the CRC32 of the piece, its length (ISIZE).  The payload is ONE deflate
 * block with BFINAL set: dynamic Huffman (BTYPE 10) over LZ77 matches of length 4..258 at distance 1..32768 that never reach
 * before the piece's first byte nor past its last -- every block inflates on its own --, code lengths of at most 15 bits, run-
 * length coded (16, 17, 18) under a code-length code of at most 7 bits; or, when that is not smaller, stored (BTYPE 00).  A
 * block is therefore never longer than its piece + 31 bytes.  The bytes are a function of (text, block_bytes) alone: not of
 * thread order, launch geometry, slab size or which of the two calls below made them.  Blocks, and files of blocks, joined end
 * to end are a valid file; kbbq_bgzf_eof writes the 28-byte empty block that ends a BGZF file.
 * kbbq_bgzf_bound(n, block_bytes) = n + 31 * ceil(n / block_bytes): what the packed blocks of n bytes can need (0 for n <= 0 or
 * a block_bytes out of range).
 * kbbq_bgzf_deflate_dev (synchronous): block b is written at d_blocks + b * KBBQ_BGZF_SLOT and its length to d_sizes[b]
 * (d_blocks: ceil(n / block_bytes) * KBBQ_BGZF_SLOT bytes; both 4-byte aligned); then the blocks are copied end to end into
 * d_packed (kbbq_bgzf_bound bytes) and *packed_bytes receives their total length.  d_text is not written; it is read fastest
 * when it and block_bytes are multiples of 16.
 * kbbq_bgzf_deflate: the same from and to host buffers, slab by slab through page-locked staging (KBBQ_STAGE_MB) like
 * kbbq_kmer_count; only text goes up and only packed bytes come back.  out_cap must be at least kbbq_bgzf_bound.
 * n == 0 writes nothing and launches nothing (*packed_bytes = *out_bytes = 0).  KBBQ_E_ARG before anything is launched: a
 * block_bytes outside 1..KBBQ_BGZF_BLOCK_MAX (checked first, on the number alone), a NULL ctx, buffer or result pointer, n < 0,
 * buffers that are not aligned as said, an out_cap below the bound.  The launches are not timed by kbbq_ctx_timing.
 * kbbq_bgzf_deflate_dev touches only scratch of its own in the context and enqueues on its stream: like the copies, it may run
 * on a second thread beside the one that launches the other kernels, one such call at a time (kbbq/_bgzf.py does).           */
#define KBBQ_BGZF_BLOCK_MAX 65280
#define KBBQ_BGZF_SLOT      65536
#define KBBQ_BGZF_EOF_BYTES 28
size_t kbbq_bgzf_bound(int64_t n, int block_bytes);
int kbbq_bgzf_deflate_dev(kbbq_ctx* ctx, const uint8_t* d_text, int64_t n, int block_bytes, uint8_t* d_blocks, uint32_t* d_sizes,
                          uint8_t* d_packed, size_t* packed_bytes);
int kbbq_bgzf_deflate(kbbq_ctx* ctx, const uint8_t* text, int64_t n, int block_bytes, uint8_t* out, size_t out_cap,
                      size_t* out_bytes);
int kbbq_bgzf_eof(uint8_t* out);

/* ---- BAM output (--bam-out; csrc/sam_host.cpp, csrc/kbbq_bam_out.h, kbbq/_bamout.py) --------------------------------------------
 * THE STREAM (SAM specification section 4.2) is defined by the SAM text T the same command writes without the option: magic,
 * the header text as read (every header line + '\n'), the references of the @SQ lines in order; per alignment block_size, refID
 * / next_refID as indices of the @SQ list ('*' -1, '=' the record's own), pos - 1, l_read_name, mapq, bin = reg2bin(pos, pos +
 * max(reference span, 1)), n_cigar_op, flag, l_seq, pnext - 1, tlen, QNAME + NUL, CIGAR as u32 (length << 4 | op), SEQ as
 * nibbles over "=ACMGRSVTWYHKDBN" (lower case like upper case, any other byte 15, the last nibble of an odd length 0), QUAL as
 * phred bytes (0xFF x l_seq for '*'), the tags in the order of the line: i as the smallest of c C s S i I that holds the value,
 * A f Z H B as written; with set_oq a record without an OQ tag and with a QUAL gets OQ:Z:<QUAL as read> as its last tag.
 * (A one-base record whose new QUAL character is '*', quality 9, reads as "no QUAL" in T: its QUAL byte is 0xFF here as well.)
 * The work is divided: the host, in parallel over records, writes what only the text knows; the device adds SEQ and QUAL from
 * the planes the apply kernel (kbbq_apply_aligned*_dev) read and wrote, so that neither crosses the bus again.
 * kbbq_bam_header: the stream's head (magic .. references); out == NULL: *used = the bytes needed.  KBBQ_E_RANGE for an @SQ line
 * without SN or a decimal LN.
 * kbbq_bam_header_text: the same head, by the same code, of header lines given as text (each line ended by '\n'; empty lines are
 * skipped) -- for a caller that has the lines but no kbbq_sam, as kbbq_bam_scan's caller has.
 * kbbq_bam_check: what BAM cannot hold, of alignments [first, first + n): an RNAME or RNEXT that is not in @SQ, a QNAME longer than
 * 254 bytes, more than 65535 CIGAR operations, an unknown CIGAR letter, a malformed tag, an integer tag outside int32 / uint32, SEQ
 * '*' with a QUAL (or a QUAL of another length than SEQ), a FLAG or MAPQ beyond its field -- KBBQ_E_RANGE, the message naming
 * the lowest such alignment and *bad_index its index; -1 and KBBQ_OK when there is none.
 * kbbq_bam_layout: one descriptor per record of a slab (alignments [first, first + n), checked before), the size of the slab's
 * compact skeleton and of its stream.  keep_qual (n bytes, or NULL for none): nonzero for a record the apply passes through --
 * its QUAL stays as read; a '*' QUAL always does.  Offsets within a slab are 32 bits: KBBQ_E_RANGE for a stream of 2^31 bytes
 * or more.
 * kbbq_bam_skeleton: the skeleton the descriptors describe: per record, at skel_off, head_bytes (block_size, the 32 fixed bytes,
 * QNAME, CIGAR), then -- qual_src == KBBQ_BAM_QUAL_SKELETON -- l_seq bytes of QUAL (as read - 33, or 0xFF), then tail_bytes (the
 * encoded tags).  No SEQ, no recalibrated QUAL.
 * kbbq_bam_assemble_dev: the slab's stream in device memory: record r at d_stream + carry + stream_off as   head | SEQ of row r of
 * d_seq packed | QUAL | tail,   QUAL = row r of d_qplane (characters, as the apply writes them) - 33, or the skeleton's bytes.
 * Rows are `pitch` bytes apart (a multiple of 16, 16-byte aligned); carry leaves room in front for what the previous slab left
 * below a whole BGZF block; stream_bytes is what d_stream holds.  Synchronous.  *bad_row = the lowest row with a new quality
 * below 0 (an output character below 33: SAM text holds it, BAM does not), -1 when there is none: the stream is then not to be
 * used.  A descriptor that reaches outside the skeleton, the stream or a row writes nothing and is KBBQ_E_ARG.
 * kbbq_bam_assemble: the same over host memory, by the same per-record code (csrc/kbbq_bam_out.h bo_record).
 * kbbq_bam_index_dev / kbbq_bam_index ("BAM index", below) read the same skeleton and descriptors after the assemble call: the
 * index of the file is reduced from them, in offsets of this stream.                                                           */
#define KBBQ_BAM_QUAL_PLANE    0
#define KBBQ_BAM_QUAL_SKELETON 1
typedef struct kbbq_bam_desc {
    uint32_t skel_off, head_bytes, tail_bytes, l_seq, stream_off, qual_src;
} kbbq_bam_desc;
int kbbq_bam_header(const kbbq_sam* f, uint8_t* out, size_t cap, size_t* used);
extern int kbbq_bam_header_text(const uint8_t* text, size_t n, uint8_t* out, size_t cap, size_t* used);
int kbbq_bam_check(const kbbq_sam* f, int64_t first, int64_t n, int64_t* bad_index);
int kbbq_bam_layout(const kbbq_sam* f, int64_t first, int64_t n, int set_oq, const uint8_t* keep_qual, kbbq_bam_desc* desc,
                    size_t* skel_bytes, size_t* stream_bytes);
int kbbq_bam_skeleton(const kbbq_sam* f, int64_t first, int64_t n, int set_oq, const kbbq_bam_desc* desc, uint8_t* skel, size_t cap);
int kbbq_bam_assemble_dev(kbbq_ctx* ctx, const uint8_t* d_skel, size_t skel_bytes, const kbbq_bam_desc* d_desc, int64_t n,
                          const uint8_t* d_seq, const uint8_t* d_qplane, int pitch, uint8_t* d_stream, size_t carry,
                          size_t stream_bytes, int64_t* bad_row);
int kbbq_bam_assemble(const uint8_t* skel, size_t skel_bytes, const kbbq_bam_desc* desc, int64_t n, const uint8_t* seq,
                      const uint8_t* qplane, int pitch, uint8_t* stream, size_t carry, size_t stream_bytes, int64_t* bad_row);

/* ---- BAM index (--bam-index; csrc/kbbq_bam_index.h, kbbq/_bamindex.py; the executable model: tests/bam_index_model.py) ---------
 * THE INDEX of a --bam-out file, BAI (SAM specification 5.2) or CSI (min_shift 14, depth the smallest >= 5 with 2^(14 + 3 *
 * depth) >= the largest LN, l_aux 0, BGZF-compressed by kbbq_bgzf_deflate* plus the EOF block).  auto: BAI when every LN <= 2^29.
 * No byte parity with samtools is claimed; the file is a valid index by the specifications, defined by these rules.
 * Record extent: beg = pos (0-based; below 0: 0), end = beg + the reference span of the CIGAR (M D N = X), at least beg + 1.  A
 * placed unmapped read (flag 4 with a refID) is indexed like any other with end = beg + 1.
 * Bin: reg2bin(beg, end, 14, depth), computed here (the record's bin field covers depth 5 only).  A record with refID < 0
 * enters no bin and counts into n_no_coor.
 * Virtual offsets: with u an absolute offset of the uncompressed stream, voffset(u) = coff[u / 65280] << 16 | u % 65280, coff[b]
 * the file offset of BGZF block b and coff[nblocks] that of the EOF block (what htslib's bgzf_tell gives behind a record that
 * ends on a block boundary).  A record's chunk is [voffset(start), voffset(start + 4 + block_size)).
 * Chunks of a bin: one per maximal run of consecutive records of one (refID, bin), in file order; neighbouring chunks of one bin
 * are then merged where the earlier one's end and the later one's begin lie in one compressed block (end >> 16 >= beg >> 16:
 * htslib's rule).  The bins of a reference are written in ascending bin number, the pseudo-bin last.
 * Linear index (BAI): ceil(max(LN, 1) / 16384) + 1 windows per reference; a window holds the lowest record-start voffset over
 * the records that overlap it, the window index clamped to the reference's last (a record overhanging LN is kept); n_intv = the
 * last non-empty window + 1; an empty window below that takes the value of the next non-empty one above it.  CSI loffset of a
 * bin: that backfilled value at the bin's first 16 kb window (clamped likewise; 0 behind the last non-empty window).
 * Metadata pseudo-bin (37450 for BAI, ((1 << (3 * depth + 3)) - 1) / 7 + 1 for CSI), for every reference with records: the pairs
 * (ref_beg, ref_end) as voffsets and (n_mapped, n_unmapped).  The file ends with n_no_coor.  A header-only BAM gives n_ref empty
 * references.  The input must be in coordinate order: (refID as unsigned, pos) non-decreasing -- checked by the caller.
 * kbbq_bam_index_dev: one slab, after kbbq_bam_assemble_dev over the same skeleton and descriptors and on the same stream.  All
 * offsets are absolute offsets of the uncompressed stream (stream_base: where the descriptors' stream_off 0 lies); the host
 * converts (monotone).  d_lin_off[n_ref + 1]: the prefix sum of the references' window counts; d_linear[d_lin_off[n_ref]]: the
 * file-long linear array, all ones before the first slab, min(start) per window after (64-bit atomicMin).  runs (host memory,
 * cap >= n entries): one 32-byte run per maximal run of one (refID, bin) within the slab, refID -1 for records without a
 * coordinate; *n_runs their number -- only they and three words come back, per-record entries never do.  The caller joins a slab's
 * first run with the last of the slab before when (refID, bin) agree.  *bad_row = the lowest row that does not fit (its head
 * outside the skeleton, its CIGAR outside its head, a refID >= n_ref, an end beyond 2^(14 + 3 * depth)), -1 when there is none;
 * such a row touches no window, the call is KBBQ_E_ARG and the runs are not to be used.  Synchronous.  depth in 5..8.
 * kbbq_bam_index: the same over host memory, by the same per-record code (csrc/kbbq_bam_index.h bix_entry).                     */
typedef struct kbbq_bam_run {
    int32_t ref; uint32_t bin;
    uint64_t beg, end;                   /* stream offsets: the first record's start, the last record's end */
    uint32_t n_mapped, n_unmapped;
} kbbq_bam_run;
extern int kbbq_bam_index_dev(kbbq_ctx* ctx, const uint8_t* d_skel, size_t skel_bytes, const kbbq_bam_desc* d_desc, int64_t n,
                              uint64_t stream_base, int depth, const uint64_t* d_lin_off, int n_ref, uint64_t* d_linear,
                              kbbq_bam_run* runs, int64_t cap, int64_t* n_runs, int64_t* bad_row);
extern int kbbq_bam_index(const uint8_t* skel, size_t skel_bytes, const kbbq_bam_desc* desc, int64_t n, uint64_t stream_base,
                          int depth, const uint64_t* lin_off, int n_ref, uint64_t* linear, kbbq_bam_run* runs, int64_t cap,
                          int64_t* n_runs, int64_t* bad_row);

/* ---- BGZF input: inflate on the GPU (csrc/kbbq_bgzf_inflate.h, csrc/bam_host.cpp kbbq_inflate_all, kbbq/_bgzf.py inflate) -------
 * A BGZF file is a row of gzip members of at most 64 KiB in and 64 KiB out, each naming its own compressed size (BSIZE), CRC32
 * and length (ISIZE): a member is one workgroup's work.
 * kbbq_inflate_index: the block table of src[0, n), from headers and trailers alone (no HIP call, nothing is inflated).  Member b:
 * its deflate payload is src[blocks[b].src, + csize), its text belongs at blocks[b].dst = the sum of the ISIZE fields before
 * it.  blocks == NULL (or cap too small: KBBQ_E_ARG) only counts: *nblocks and *text_bytes are set either way.  Returns
 * KBBQ_INFLATE_NOT_BGZF (no error text) for anything that is not BGZF from its first to its last byte: a member without the BC
 * subfield, a BSIZE that runs past n, an ISIZE above 65536.  Such a stream stays on the caller's host path.
 * kbbq_inflate_bgzf_dev (synchronous): kernel bi_inflate over nblocks members, everything in device memory.  d_blocks are
 * descriptors as above with offsets into d_src (src_bytes long) and d_out (out_bytes long); d_status[b] receives 0 and the text
 * lies at d_out + dst, or a KBBQ_INFLATE_* value above 0 and NOTHING of d_out was written for that member: a descriptor that
 * reaches outside either buffer, a bad block type, an over-subscribed or incomplete code, literal/length symbol 286 / 287 or
 * distance symbol 30 / 31, a distance before the member's start, output past ISIZE, input past the payload, a stored block
 * whose LEN and NLEN disagree, text shorter than ISIZE, payload bytes behind the last deflate block, a CRC32 other than the
 * trailer's.  All of RFC 1951 is decoded (stored, fixed and dynamic blocks in any number, codes of up to 15 bits, lengths 3..258,
 * distances 1..32768, overlapping copies, the empty member).  A status is not a verdict on the data: the kernel never decides
 * that a file is damaged, the caller inflates such a member again on the host.
 * kbbq_inflate_bgzf: the same from and to host buffers, slab by slab (whole members) through the context's page-locked staging
 * (KBBQ_STAGE_MB): compressed bytes go up, text comes down.  Members with a status are inflated again on the host inside the
 * call, as kbbq_inflate_all does it (libdeflate, then zlib); when that fails too the call fails with KBBQ_E_ARG and the reader's
 * error text.  *text_bytes = the bytes written to out (out_cap must hold the sum of the ISIZE fields).  stats (may be NULL).
 * kbbq_inflate_bgzf_host: the decoder of the kernel (bi_member), compiled for the host, on ONE member: payload[0, n) into
 * out[0, isize); returns the status the kernel would give.  Writes out[0, isize) only.  For tests and fuzzing.
 * kbbq_inflate_use_ctx: the context the readers (kbbq_fastq_open, kbbq_text_open, kbbq_sam_open: csrc/bam_host.cpp kbbq_inflate_all)
 * may use, or NULL for none; kbbq_ctx_destroy takes it back.  The device route is taken when a context is registered,
 * KBBQ_GPU_INFLATE is 1 (the default is the host route: profiles/bgzf_inflate.md), the stream indexes as BGZF and is at least
 * KBBQ_GPU_INFLATE_MIN_BYTES long (default 1 MiB); a failure of the route other than damaged data falls back to the host route.
 * The route has staging and a stream of its own in the context and takes a lock: readers on several threads take turns.
 * kbbq_inflate_stats_get: what the readers sent that way since the process began.
 * KBBQ_E_ARG before any HIP call: a NULL ctx, a NULL buffer or result pointer with something to do, d_blocks not 8-byte or
 * d_status not 4-byte aligned, nblocks < 0 or above 2^31 - 1, an out_cap below the text.  nblocks == 0 launches nothing.        */
#define KBBQ_INFLATE_NOT_BGZF 1
enum {
    KBBQ_INFLATE_OK = 0, KBBQ_INFLATE_BTYPE, KBBQ_INFLATE_CODE, KBBQ_INFLATE_SYMBOL, KBBQ_INFLATE_DISTANCE, KBBQ_INFLATE_OUTPUT,
    KBBQ_INFLATE_INPUT, KBBQ_INFLATE_STORED, KBBQ_INFLATE_ISIZE, KBBQ_INFLATE_TRAILING, KBBQ_INFLATE_CRC, KBBQ_INFLATE_RANGE,
    KBBQ_INFLATE_TABLE
};
typedef struct kbbq_bgzf_block {
    uint64_t src, dst;                /* the payload's offset in the compressed bytes, the text's in the output */
    uint32_t csize, isize, crc, pad;  /* payload bytes, ISIZE, CRC32 */
} kbbq_bgzf_block;
typedef struct kbbq_inflate_stats {
    uint64_t device_blocks, host_blocks, bytes_up, bytes_down;   /* inflated by the kernel, redone on the host, over the bus */
} kbbq_inflate_stats;
int kbbq_inflate_index(const uint8_t* src, size_t n, kbbq_bgzf_block* blocks, size_t cap, size_t* nblocks, size_t* text_bytes);
int kbbq_inflate_bgzf_dev(kbbq_ctx* ctx, const uint8_t* d_src, size_t src_bytes, const kbbq_bgzf_block* d_blocks, int64_t nblocks,
                          uint8_t* d_out, size_t out_bytes, uint32_t* d_status);
int kbbq_inflate_bgzf(kbbq_ctx* ctx, const uint8_t* src, size_t n, uint8_t* out, size_t out_cap, size_t* text_bytes,
                      kbbq_inflate_stats* stats);
int kbbq_inflate_bgzf_host(const uint8_t* payload, uint32_t n, uint8_t* out, uint32_t isize, uint32_t crc);
int kbbq_inflate_use_ctx(kbbq_ctx* ctx);
int kbbq_inflate_stats_get(kbbq_inflate_stats* stats);

/* ---- BAM input: records decoded on the GPU (csrc/bam_host.cpp kbbq_bam_scan, csrc/kbbq_bam_in.h, kbbq/_bamin.py) ----------------
 * For the commands that write no record (bqsr --kmers, count -b) the SAM text the host reader renders from a BAM file serves
 * nothing: a kernel turns the uploaded records into the resident planes and per-record words.  The host reader (kbbq_sam_open)
 * stays the reference: what the decode writes is what the reader's arrays hold for the same record, or a status bit, and a file
 * with a status bit anywhere -- or with a scan error -- is the reader's to read or to refuse.
 * kbbq_bam_scan: an inflated BAM image (magic .. last record).  With every array NULL it fills *info only; the caller sizes the
 * arrays from it and calls again.  header[header_bytes]: the header lines exactly as kbbq_bam_to_sam writes them in front of the
 * records (NUL padding stripped, a final '\n' added, @SQ lines made from the binary list when the text has none); rg_off[n_rg + 1]
 * / rg_ids[rg_bytes]: the ID of every @RG line in header order (the line's last ID: field, empty without one); rec_off[n]: the
 * offset of every record's body (behind its block_size word) in the image; cig_off[n + 1]: the running sum of n_cigar_op.
 * info: n, cig_total, max_l_seq (the longest l_seq, negative ones taken as 0), n_ref, n_rg, header_bytes, rg_bytes, refs_off (of
 * the binary reference list: n_ref times l_name, name, l_ref), records_off (of the first block_size word), max_record (the
 * largest block_size + 4).  KBBQ_E_ARG with the reader's own text for a defect: "not a BAM file", "BAM header text runs past the
 * file", "BAM reference list runs past the file", "BAM: negative reference count", "BAM: truncated record".
 * kbbq_bam_decode_dev (synchronous) / kbbq_bam_decode (the same over host memory, by the same per-record code: bd_record): m
 * records of a slab -- a piece of the image that holds whole records, each behind its block_size word -- into rows [0, m) of
 * the planes and words [0, m).  rec_off[m]: the bodies' offsets in the slab; cig_off[m + 1]: the records' ranges in `cigar` (of
 * cig_cap words).  pitch: a multiple of 16 in 16..65536; planes 16-byte aligned.  seq / qual / oq / words / cigar may each be
 * NULL: it is not written.  Every byte of rows [0, m) x pitch, every word and every word of the CIGAR ranges is written: nothing
 * needs zeroing first.  Planes hold what kbbq_sam_fill writes: SEQ letters, QUAL + 33 (zeros for an absent QUAL: l_seq 0, a
 * first byte of 0xFF, or ONE quality of 9, which the text shows as '*'), the value of the last OQ:Z tag; truncated at pitch, zero
 * padded.  Words: kbbq_bam_words, with the meanings of kbbq_sam_fields (pos / pnext 0-based; oq_len -1 without a tag; rg the index
 * of the FIRST @RG line with the ID of the LAST RG:Z tag, -1 without a tag, -2 for an ID the header lacks; trim:
 * kbbq_sam_adaptor_trim's word); ref_id as stored.  status != 0: the record is not vouched for -- its rows and CIGAR words are zeros
 * and its other words 0:
 *   KBBQ_BAM_ST_RECORD  inconsistent by the reader's own tests (l_seq < 0, l_read_name 0, the fixed parts or a tag overrun the
 *                       record, QNAME without its NUL, a refID / next_refID >= n_ref, an unknown tag type or B subtype)
 *   KBBQ_BAM_ST_LONG    l_seq above 65535, an OQ value above 32767 (the longest kbbq_sam_fields takes)
 *   KBBQ_BAM_ST_QUAL    a present QUAL with a byte above 93
 *   KBBQ_BAM_ST_TEXT    the rendered line would split differently or hold another value: a byte outside 0x21..0x7E in the RG or
 *                       OQ value or a tag's name, a byte below 0x20 in QNAME, in an A value or in any Z / H value, a QNAME that
 *                       begins with '@', a CIGAR operation above 8
 *   KBBQ_BAM_ST_RANGE   the record (its block_size word included) does not lie in the slab, or its CIGAR range is not
 *                       n_cigar_op words inside cigar[0, cig_cap)
 * *any_status: the OR of all of them.  Whatever the bytes, nothing outside the slab is read and nothing outside the rows, the
 * words and the CIGAR ranges is written; every length is checked against the record's end in 64-bit arithmetic before it is
 * used; no read passes a record's end (the last chunk of a field is read bytewise), so the slab needs no slack.
 * KBBQ_E_ARG before any HIP call: a NULL ctx, slab, rec_off or any_status with m > 0, cigar without cig_off, n_rg > 0 without the
 * table, m outside 0..2^31 - 1, a slab of 2^32 bytes or more, a bad pitch or alignment.                                        */
#define KBBQ_BAM_ST_RECORD 1u
#define KBBQ_BAM_ST_LONG   2u
#define KBBQ_BAM_ST_QUAL   4u
#define KBBQ_BAM_ST_TEXT   8u
#define KBBQ_BAM_ST_RANGE  16u
typedef struct kbbq_bam_scan_info {
    int64_t n, cig_total;
    int32_t max_l_seq, n_ref, n_rg, pad;
    uint64_t header_bytes, rg_bytes, refs_off, records_off, max_record;
} kbbq_bam_scan_info;
typedef struct kbbq_bam_words {
    int32_t flag, ref_id, pos, pnext, tlen, qlen, qual_len, oq_len, rg, cig_n, ref_span;
    uint32_t clip, trim, status, pad[2];
} kbbq_bam_words;
extern int kbbq_bam_scan(const uint8_t* image, size_t n, kbbq_bam_scan_info* info, uint8_t* header, uint32_t* rg_off, uint8_t* rg_ids,
                  uint64_t* rec_off, uint64_t* cig_off);
extern int kbbq_bam_decode_dev(kbbq_ctx* ctx, const uint8_t* d_slab, size_t slab_bytes, const uint32_t* d_rec_off, int64_t m, int pitch,
                        const uint32_t* d_rg_off, const uint8_t* d_rg_ids, int n_rg, int n_ref, const uint32_t* d_cig_off,
                        size_t cig_cap, uint8_t* d_seq, uint8_t* d_qual, uint8_t* d_oq, kbbq_bam_words* d_words, uint32_t* d_cigar,
                        uint32_t* any_status);
extern int kbbq_bam_decode(const uint8_t* slab, size_t slab_bytes, const uint32_t* rec_off, int64_t m, int pitch, const uint32_t* rg_off,
                    const uint8_t* rg_ids, int n_rg, int n_ref, const uint32_t* cig_off, size_t cig_cap, uint8_t* seq, uint8_t* qual,
                    uint8_t* oq, kbbq_bam_words* words, uint32_t* cigar, uint32_t* any_status);

/* ---- BAM recode: the --bam-out skeleton from resident BAM records (csrc/kbbq_bam_recode.h, kbbq/_bamin.py, kbbq/_bamout.py) ------
 * BAM in, BAM out: the records kbbq_bam_decode_dev read hold every byte of the skeleton kbbq_bam_skeleton writes from the SAM
 * text of the same records, but for the `bin` field (computed), integer tags (the text route stores each in the first type of
 * c C s S i I that holds its value) and an absent QUAL (0xFF throughout).  The host route -- kbbq_sam_open on the text of the
 * records, then kbbq_bam_layout and kbbq_bam_skeleton -- stays the reference: what the recode writes is what those two write, or
 * a status bit.
 * kbbq_bam_recode_dev (synchronous) / kbbq_bam_recode (the same over host memory, by the same per-record code: br_size,
 * br_write): records [first, first + m) of an inflated BAM image.  rec_off: kbbq_bam_scan's array of the WHOLE image (64-bit
 * offsets of the records' bodies; entries [first, first + m) are read).  set_oq, keep (m bytes, nonzero: QUAL stays as read; NULL:
 * none) and n_ref as kbbq_bam_layout / kbbq_bam_decode take them.  Written: desc[0, m) (the m descriptors of kbbq_bam_layout),
 * status[0, m), skel[0, *skel_bytes) (the skeleton of kbbq_bam_skeleton), *skel_bytes, *stream_bytes, *any_status (the OR of the
 * status words).  The offsets are an exclusive scan done on the device.  skel == NULL (skel_cap 0): everything but the skeleton.
 * status != 0: the record's text round trip is not provably the identity -- its descriptor is zeros (it takes no room in the
 * skeleton or the stream) and nothing of it is written; the caller hands the file to the host route.  The bits are the decode's
 * (KBBQ_BAM_ST_RECORD .. KBBQ_BAM_ST_RANGE, decided by the decode's own code on the same bytes; RANGE: the record does not lie in
 * the image) and
 *   KBBQ_BAM_ST_FLOAT   an `f` tag or a B:f array (the reader renders floats with %g)
 *   KBBQ_BAM_ST_REF     a refID or next_refID below -1 (the reader shows every negative one as '*', which is written as -1)
 * refID / next_refID are otherwise kept as stored: the caller sees to it that the header's @SQ lines name the binary reference
 * list in order.  Whatever the bytes, nothing outside the image is read, nothing outside desc[0, m), status[0, m) and
 * skel[0, *skel_bytes) is written, and every length is checked against the record's end in 64-bit arithmetic before it is used.
 * KBBQ_E_RANGE: a stream of 2^31 bytes or more (offsets are 32 bits), as kbbq_bam_layout; the skeleton is not written.
 * KBBQ_E_ARG: a skeleton larger than skel_cap (*skel_bytes says how large; the skeleton is not written); and, before any HIP
 * call, a NULL ctx, buffer or result pointer, first < 0, m outside 0..2^31 - 1, n_ref < 0, a bad alignment (rec_off 8 bytes,
 * desc / status 4).                                                                                                             */
#define KBBQ_BAM_ST_FLOAT  32u
#define KBBQ_BAM_ST_REF    64u
extern int kbbq_bam_recode_dev(kbbq_ctx* ctx, const uint8_t* d_image, size_t image_bytes, const uint64_t* d_rec_off, int64_t first,
                        int64_t m, int set_oq, const uint8_t* d_keep, int n_ref, kbbq_bam_desc* d_desc, uint8_t* d_skel,
                        size_t skel_cap, uint32_t* d_status, size_t* skel_bytes, size_t* stream_bytes, uint32_t* any_status);
extern int kbbq_bam_recode(const uint8_t* image, size_t image_bytes, const uint64_t* rec_off, int64_t first, int64_t m, int set_oq,
                    const uint8_t* keep, int n_ref, kbbq_bam_desc* desc, uint8_t* skel, size_t skel_cap, uint32_t* status,
                    size_t* skel_bytes, size_t* stream_bytes, uint32_t* any_status);

#ifdef __cplusplus
}
#endif
#endif /* KBBQ_HIP_H */
