// kbbq_quantize_kernels.h -- static quantized qualities (--static-quantized-quals) on a byte plane, in place.
//
// The rule is a byte map qmap[256] over OUTPUT bytes (include/kbbq_hip.h "Static quantized qualities"; kbbq/gatk/applybqsr.py
// quantize_map builds it): identity below 33 + minscore -- padding zeros, the separator of a mate-pair row, preserved bases, a new
// quality below minscore -- and every other byte to the level of E = {minscore} U levels it rounds to.  So the kernel knows nothing
// of rows, lengths or layouts: character rows, mate-pair rows and planes K2 stored back in input order are all byte planes whose
// padding is zero, and qmap[0] == 0.
//   kq_plane   d_plane[i] = qmap[d_plane[i]] over nbytes (a multiple of 16; 16-byte aligned): one lane per 16-byte chunk per step
//              of a grid-stride walk, 16-byte loads and stores, the table in LDS (256 bytes per workgroup, one byte per thread)
// It runs after K2 on K2's stream.  K2's output byte is the SUM of two LUT entries (cycle + context), so the map cannot be folded
// into either entry; K2 and its LUTs stay as they are, and this is one more pass of 1 byte read + 1 byte written per base.
// The table is read with 16 ds_read_u8 per chunk: 64 lanes x 1 byte per wave-instruction against a 64-dword table, where lanes
// that name the same byte (a handful of levels: the usual case) are served by one broadcast.
#pragma once
#include "kbbq_helpers.h"

#define KQ_THREADS 256
#define KQ_CHUNKS_PER_LANE 8         // grid sizing: a workgroup walks at least this many 4 KB tiles when the plane is large

// the 256-byte table, one byte per thread of a 256-thread workgroup; the barrier is the caller's
__device__ __forceinline__ void kq_stage(uint8_t* tab, const uint8_t* __restrict__ qmap)
{
    static_assert(KQ_THREADS == 256, "one table byte per thread");
    tab[threadIdx.x] = qmap[threadIdx.x];
}

__device__ __forceinline__ u32 kq_word(const uint8_t* tab, u32 w)
{
    return (u32)tab[w & 0xFFu] | ((u32)tab[(w >> 8) & 0xFFu] << 8) | ((u32)tab[(w >> 16) & 0xFFu] << 16) | ((u32)tab[w >> 24] << 24);
}

__global__ __launch_bounds__(KQ_THREADS) void kq_plane(uint8_t* __restrict__ plane, long long nchunks, const uint8_t* __restrict__ qmap)
{
    __shared__ uint8_t tab[256];
    kq_stage(tab, qmap);
    __syncthreads();
    uint4* p = reinterpret_cast<uint4*>(plane);
    const long long step = (long long)gridDim.x * KQ_THREADS;
    for (long long i = (long long)blockIdx.x * KQ_THREADS + threadIdx.x; i < nchunks; i += step) {
        const uint4 v = p[i];
        p[i] = make_uint4(kq_word(tab, v.x), kq_word(tab, v.y), kq_word(tab, v.z), kq_word(tab, v.w));
    }
}
