// kbbq_helpers.h -- what the kernel headers share and no kernel: the tables' constants, the status words and the device
// helpers of the byte-parallel K1 / K2 code (a unit that needs only these includes no kernel with them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define KQ      43          // maxscore + 1 (recalibrate.py:36)
#define KND     16          // dinucleotides

// status words (device, unsigned long long[KBBQ_NSTATUS], decoded by kbbq_ctx_status): min read index per error class
#define ST_INDEX 0
#define ST_TYPE  1
#define ST_RANGE 2
#define ST_LUT   3   // set (to 0) when a device-built LUT needs the checked apply kernel
#define ST_MEANQ 4   // status word: a read group whose meanq the all-device solve cannot decide (see k3_levels_ab)
#define ST_KMER  5   // status word: a k-mer insert found no free slot (kbbq_ctx_status -> KBBQ_E_FULL)
constexpr int KM_MAX_PROBES = 512;   // kbbq_kmer.h: the probes of an insert or a lookup (kbbq_ctx_status names the number)

typedef unsigned long long u64;
typedef unsigned int u32;

// ---------------------------------------------------------------- helpers
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// wave_shr:1 -- every lane receives lane-1's value, lane 0 receives `lane0`.
__device__ __forceinline__ u32 wave_shr1(u32 v, u32 lane0)
{
    return (u32)__builtin_amdgcn_update_dpp((int)lane0, (int)v, 0x138, 0xF, 0xF, false);
}

__device__ __forceinline__ u32 bperm(u32 v, int src_lane)
{
    return (u32)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

// byte-parallel nucleotide decoding of 4 bases (one 32-bit word of the seq plane).
//   h      = bits 1..3 of every byte:  A->0 C->1 T->2 G->3 N->7   (others 4,5,6 or aliases)
//   expect = the character that h stands for; a byte is in the alphabet iff expect == byte
//   code   = reference order A0 T1 G2 C3 (compare_reads.py:199), 0x10 for N / other
__device__ __forceinline__ void decode4(u32 w, u32& expect, u32& code)
{
    const u32 h = (w >> 1) & 0x07070707u;
    expect = __builtin_amdgcn_perm(0x4E000000u, 0x47544341u, h);
    code   = __builtin_amdgcn_perm(0x10101010u, 0x02010300u, h);
}

// mask with 0xFF in byte k iff (4*wd + k) < nb
__device__ __forceinline__ u32 byte_mask(int nb, int wd)
{
    const int m = nb - 4 * wd;
    return m >= 4 ? 0xFFFFFFFFu : (m <= 0 ? 0u : ((1u << (8 * m)) - 1u));
}

// (the plain load first: a status word only ever decreases, so a value already <= `read` -- however stale the copy this lane sees --
//  means the atomic could not change it.  Without it a batch in which EVERY chunk is flagged -- qualities in another encoding, a
//  kernel run twice over its own output -- spends a second in same-address atomics: 1 010 ms for 50 M reads, measured on K2.)
__device__ __forceinline__ void flag(u64* status, int which, long long read)
{
    if (__hip_atomic_load(&status[which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (u64)read) atomicMin(&status[which], (u64)read);
}

// Exact restatement of the reference's TypeError condition for one chunk
// (compare_reads.py:281-293): a dinucleotide (i-1, i) is looked up iff i >= 1,
// q[i] >= minscore and neither base is 'N'; the lookup fails when either base is
// outside ACGT.  Only reached when the cheap alphabet test fired.
__device__ __noinline__ bool chunk_type_error(u32 s0, u32 s1, u32 s2, u32 s3,
                                              u32 q0, u32 q1, u32 q2, u32 q3, u32 prevchar,
                                              int nb, int pos0, int minscore)
{
    const u32 s[4] = {s0, s1, s2, s3};
    const u32 q[4] = {q0, q1, q2, q3};
    u32 prev = prevchar;
    for (int i = 0; i < nb && i < 16; ++i) {
        const u32 ch = (s[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const int qq = (int)((q[i >> 2] >> (8 * (i & 3))) & 0xFFu) - 33;
        const bool looked = (pos0 + i) >= 1 && qq >= minscore && ch != 'N' && prev != 'N';
        const bool okc = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
        const bool okp = prev == 'A' || prev == 'C' || prev == 'G' || prev == 'T';
        if (looked && !(okc && okp)) return true;
        prev = ch;
    }
    return false;
}

// LUT (int16), one row of `rs` entries per (read group, quality):
//     row[0 .. S2-1]      = meanq + rgdq + qdq + posdq[cycle]          (lut1)
//     row[S2 .. S2+24]    = dinucdq[5 * code(prev) + code(cur)]        (lut2, code N/none = 4:
//                           every entry that involves code 4 holds dinucdq[..., -1])
// rs = lut_row_stride(S2): rs / 2 is odd so that consecutive rows start on different banks.
__host__ __device__ __forceinline__ int lut_row_stride(int S2)
{
    int rs = (S2 + 25 + 1) & ~1;
    if (((rs >> 1) & 1) == 0) rs += 2;
    return rs;
}

// Exact per-base restatement of compare_reads.py:320-328 for ONE chunk, used whenever the
// fast path cannot be taken (read group / quality / cycle beyond the tables).  Reads the LUT
// from global memory.  Returns the 16 output bytes through o[4].
__device__ __noinline__ uint4 chunk_apply_exact(const int16_t* lut, int rs, int R, int Qt, int S2,
                                               u32 qlo, int rg, bool second, int pos0, int nb,
                                               u32 q0, u32 q1, u32 q2, u32 q3,
                                               u32 d0, u32 d1, u32 d2, u32 d3,
                                               u64* status, long long read)
{
    const u32 q[4] = {q0, q1, q2, q3};
    const u32 d5[4] = {d0, d1, d2, d3};
    u32 o[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i) {
        const u32 qb = (q[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        u32 ob = qb;
        if (i < nb && qb >= qlo) {
            const int qq = (int)qb - 33;
            const int pos = pos0 + i;
            const int col = second ? (S2 - 1 - pos) : pos;           // Python wrap of -(i+1) on S2
            if (rg >= R || qq >= Qt || col < 0 || col >= S2) flag(status, ST_INDEX, read);
            else {
                const int16_t* row = lut + ((size_t)rg * Qt + qq) * rs;
                const int v = (int)row[col] + (int)row[S2 + (int)((d5[i >> 2] >> (8 * (i & 3))) & 0xFFu)] + 33;
                if (v < 0 || v > 255) flag(status, ST_RANGE, read);
                ob = (u32)v & 0xFFu;
            }
        }
        if (i >= nb) ob = 0u;
        o[i >> 2] |= ob << (8 * (i & 3));
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}
