// kbbq_byte_window.h -- 16-byte windows of a byte plane as four 32-bit words: the helpers K4 / K6 (kbbq_aligned_kernels.h) and the
// layout passes (kbbq_layout_kernels.h) share.  No kernel.
#pragma once
#include "kbbq_kernels_v3.h"

// load16_any (kbbq_kernels_v3.h) for windows that may run past the end of the array (`limit` = its size in bytes): bytes past
// the end read as zero.  Only the last chunk of the last rows / of the genome ever takes the byte path.
__device__ __forceinline__ void load16_upto(const uint8_t* base, long long off, long long limit, u32 out[4])
{
    if (off + 16 <= limit) { load16_any(base, off, out); return; }
    out[0] = out[1] = out[2] = out[3] = 0u;
    for (int b = 0; b < 16 && off + b < limit; ++b) out[b >> 2] |= (u32)base[off + b] << (8 * (b & 3));
}

// 0xFF in the bytes of word w (of a 16-byte vector) whose position p = 4w + k lies in [lo, hi)
__device__ __forceinline__ u32 range_mask(int lo, int hi, int w) { return byte_mask(hi, w) & ~byte_mask(lo, w); }

__device__ __forceinline__ void shr_bytes16(u32 v[4], int nb)            // byte i <- byte i + nb (0 <= nb <= 15), zero fill
{
    const int ws = nb >> 2; const u32 bs = (u32)(nb & 3) * 8u;
    const u32 a0 = ws == 0 ? v[0] : ws == 1 ? v[1] : ws == 2 ? v[2] : v[3];
    const u32 a1 = ws == 0 ? v[1] : ws == 1 ? v[2] : ws == 2 ? v[3] : 0u;
    const u32 a2 = ws == 0 ? v[2] : ws == 1 ? v[3] : 0u;
    const u32 a3 = ws == 0 ? v[3] : 0u;
    v[0] = __builtin_amdgcn_alignbit(a1, a0, bs); v[1] = __builtin_amdgcn_alignbit(a2, a1, bs);
    v[2] = __builtin_amdgcn_alignbit(a3, a2, bs); v[3] = a3 >> bs;
}
