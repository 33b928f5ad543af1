// kbbq_apply_aligned.h -- ApplyBQSR on aligned rows (gatk/applybqsr.py:65-78, recalibrate_bamread), the whole batch at once.
//
// Rows are the SAM reader's character planes (kbbq_sam_fill) exactly as they sit in the file: SEQ, QUAL and the OQ tag, one
// alignment per row of `pitch` bytes, zero padded, in ALIGNED orientation.  Nothing is flipped: a reverse-strand row is read
// backwards in place.  For base i of a row of length L (sequencing index j = i forward, L - 1 - i reverse):
//   source q   = the row's source plane (QUAL or OQ) - 33; bases with q < minscore keep their byte
//   cycle      = j (first of pair) or -(j + 1) (second), a negative cycle wrapping on the S2 axis as a Python index does;
//                j >= S2 on a base that is looked up -> IndexError
//   context    = the dinucleotide in sequencing orientation from the CONTEXT plane (OQ; minscore fixed at 6): reverse rows
//                take comp(s[i]) after comp(s[i + 1]) (letters other than ACGT complement to N), forward rows s[i] after s[i - 1]
//                unmapped (a letter outside ACGTN in a looked-up pair -> TypeError, compare_reads.py:281-293); none at j = 0,
//                next to an N or where the context quality is below 6 (the zero column of get_delta_qs)
//   new q      = trunc(meanq + rgdq + qdq[q] + dinucdq[q][ctx] + posdq[q][cycle]), no clipping; byte = new q + 33
//                (outside 0..255 -> KBBQ_E_RANGE, the FASTQ path's rule)
// Two forms of the model, chosen by the host (kbbq/gatk/applybqsr.py proves which one is exact):
//   AA_LUT  the int16 canonical rows of kbbq_build_lut's blob: row[cycle column] + row[S2 + 5 prev + cur]
//   AA_F64  float64 rows [base = meanq + rgdq + qdq, dinucdq[0..16], posdq[0..S2-1]] per (read group, quality): the
//           reference's own float sum, (base + dinuc) + pos, truncated by v_cvt_i32_f64 -- for models whose float sum does
//           not decompose into two integer entries (levels a few ulps off an integer, negative totals)
// Work: one lane per 16-byte chunk, lanes of a wave on consecutive chunks of consecutive rows, every plane read and written
// with full-width 16-byte accesses; the byte before / after a chunk (the forward / reverse neighbour) comes from the next
// lane over by DPP (wave_shr:1 / wave_shl:1), from memory only at the wave's two ends.
// QMAP (static quantized qualities, kbbq_quantize_kernels.h): a new byte that has passed the range check goes through the
// 256-byte map, staged in LDS once per workgroup, before it is packed into the 16-byte store.  The statuses are decided on the
// unquantized value; a preserved byte never meets the map (the map is the identity there anyway).  Without QMAP the kernel is
// the one it was: no LDS, no barrier.
#pragma once
#include "kbbq_helpers.h"
#include "kbbq_quantize_kernels.h"

#define AA_LUT 0
#define AA_F64 1
#define AA_THREADS 256
#define AA_F64_FIXED 18        // base + 17 dinucleotide columns ahead of the cycle columns of an AA_F64 row

// meta word of a row
#define AA_LEN(m)     ((m) & 0xFFFFu)
#define AA_RG(m)      (((m) >> 16) & 0xFFFu)
#define AA_SRC_OQ     (1u << 28)     // the source plane is the OQ plane (else QUAL)
#define AA_CTX_OQ     (1u << 29)     // the context plane is the OQ plane (else QUAL)
#define AA_REVERSE    (1u << 30)     // FLAG 16
#define AA_READ2      (1u << 31)     // FLAG 128

struct AaParams {
    const uint8_t* seq; const uint8_t* qual; const uint8_t* oq; const u32* meta;
    u32 nchunks; int cpr; int pitch; long long row0;      // row0: index of the launch's first row within the call (status words)
    int Qt; int S2; int minscore;
    const int16_t* lut; int rs;                          // AA_LUT: canonical rows of kbbq_lut_row_stride(S2) entries
    const double* f64; int rs64;                         // AA_F64: rows of AA_F64_FIXED + S2 doubles
    uint8_t* out; u64* status;
    const uint8_t* qmap;                                 // QMAP: the 256-byte map of the new bytes
};

// wave_shl:1 -- every lane receives lane+1's value, lane 63 receives `lane63` (the mirror of kbbq_kernels.h wave_shr1)
__device__ __forceinline__ u32 wave_shl1(u32 v, u32 lane63)
{
    return (u32)__builtin_amdgcn_update_dpp((int)lane63, (int)v, 0x130, 0xF, 0xF, false);
}

// reference order A0 T1 G2 C3; 4 = N; -1 = any other letter
__device__ __forceinline__ int aa_code(u32 c)
{
    return c == 'A' ? 0 : c == 'T' ? 1 : c == 'G' ? 2 : c == 'C' ? 3 : c == 'N' ? 4 : -1;
}

// Dinucleotide.complement.get(x, 'N') as a code: A<->T, G<->C, everything else N
__device__ __forceinline__ int aa_comp_code(u32 c)
{
    return c == 'A' ? 1 : c == 'T' ? 0 : c == 'G' ? 3 : c == 'C' ? 2 : 4;
}

__device__ __forceinline__ u32 aa_byte(const u32 (&w)[4], int b) { return (w[b >> 2] >> (8 * (b & 3))) & 0xFFu; }

template <int MODE, bool QMAP = false>
__global__ __launch_bounds__(AA_THREADS) void kaa_apply(AaParams p)
{
    __shared__ uint8_t tab[QMAP ? 256 : 1];
    if constexpr (QMAP) {
        static_assert(AA_THREADS == KQ_THREADS, "kq_stage: one table byte per thread");
        kq_stage(tab, p.qmap);
        __syncthreads();
    }
    const u32 c0 = blockIdx.x * AA_THREADS + threadIdx.x;
    const bool live = c0 < p.nchunks;
    const u32 c = live ? c0 : p.nchunks - 1;                 // every lane takes part in the DPP exchanges below
    const u32 row = c / (u32)p.cpr, k = c - row * (u32)p.cpr;
    const u32 m = p.meta[row];
    const int L = (int)AA_LEN(m);
    const size_t at = (size_t)row * p.pitch + 16u * k;
    const uint4 sv = *reinterpret_cast<const uint4*>(p.seq + at);
    const uint4 qv = *reinterpret_cast<const uint4*>(((m & AA_SRC_OQ) ? p.oq : p.qual) + at);
    const bool same = !(m & AA_SRC_OQ) == !(m & AA_CTX_OQ);
    uint4 cv = qv;
    if (!same) cv = *reinterpret_cast<const uint4*>(((m & AA_CTX_OQ) ? p.oq : p.qual) + at);
    // the neighbours: the last byte of the chunk before (forward rows) and the first byte of the chunk after (reverse rows)
    const int lane = lane_id();
    u32 edge_prev = 0, edge_next = 0;
    if (lane == 0 && k > 0) edge_prev = p.seq[at - 1];
    if (lane == 63 && k + 1 < (u32)p.cpr) edge_next = p.seq[at + 16];
    const u32 prev_w = wave_shr1(sv.w, edge_prev << 24);
    const u32 next_w = wave_shl1(sv.x, edge_next);
    // a neighbour that belongs to another row is never looked at: i = 0 / i = L - 1 have no previous base in sequencing order
    if (!live) return;
    const u32 s[4] = {sv.x, sv.y, sv.z, sv.w}, q[4] = {qv.x, qv.y, qv.z, qv.w}, cq[4] = {cv.x, cv.y, cv.z, cv.w};
    const bool rev = m & AA_REVERSE, r2 = m & AA_READ2;
    const int rg = (int)AA_RG(m);
    const u32 qlo = 33u + (u32)p.minscore;
    const long long read = p.row0 + (long long)row;
    bool bad_type = false, bad_index = false, bad_range = false;
    u32 o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const int i = 16 * (int)k + b;
        if (i >= L) continue;
        const u32 sb = aa_byte(s, b), qb = aa_byte(q, b), cb = aa_byte(cq, b);
        const u32 nb = b == 15 ? (next_w & 0xFFu) : aa_byte(s, b + 1);
        const u32 pb = b == 0 ? (prev_w >> 24) : aa_byte(s, b - 1);
        const int j = rev ? L - 1 - i : i;
        // context in sequencing orientation
        int cur, prv;
        if (rev) { cur = aa_comp_code(sb); prv = aa_comp_code(nb); }
        else { cur = aa_code(sb); prv = aa_code(pb); }
        const bool ctx_ok = j >= 1 && cb >= 39u && cur != 4 && prv != 4;
        if (ctx_ok && (cur < 0 || prv < 0)) bad_type = true;
        u32 nq = qb;
        if (qb >= qlo) {
            const int qq = (int)qb - 33;
            if (qq >= p.Qt || j >= p.S2) { bad_index = true; nq = 0; }
            else {
                const int col = r2 ? p.S2 - 1 - j : j;
                const bool ctx = ctx_ok && cur >= 0 && prv >= 0;
                int v;
                if constexpr (MODE == AA_LUT) {
                    const int16_t* lr = p.lut + (size_t)(rg * p.Qt + qq) * p.rs;
                    v = (int)lr[col] + (int)lr[p.S2 + (ctx ? 5 * prv + cur : 24)];
                } else {
                    const double* fr = p.f64 + (size_t)(rg * p.Qt + qq) * p.rs64;
                    const double sum = (fr[0] + fr[1 + (ctx ? 4 * prv + cur : 16)]) + fr[AA_F64_FIXED + col];
                    v = (sum > -1.0e9 && sum < 1.0e9) ? (int)sum : 1 << 30;      // (int) truncates toward zero, as astype(np.int_)
                }
                const int byte = v + 33;
                if (byte < 0 || byte > 255) { bad_range = true; nq = 0; }
                else if constexpr (QMAP) nq = tab[byte];
                else nq = (u32)byte;
            }
        }
        o[b >> 2] |= nq << (8 * (b & 3));
    }
    *reinterpret_cast<uint4*>(p.out + at) = make_uint4(o[0], o[1], o[2], o[3]);
    if (bad_type) flag(p.status, ST_TYPE, read);
    if (bad_index) flag(p.status, ST_INDEX, read);
    if (bad_range) flag(p.status, ST_RANGE, read);
}
