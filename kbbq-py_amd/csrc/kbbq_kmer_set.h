// K-mer sets (kbbq count, --kmers-from; kbbq/kmerset.py): the pair check of a saved set's slabs.
//
// A k-mer set file holds the (canonical key, count) pairs with count >= keep of a finished count, ascending by unsigned key
// (include/kbbq_hip.h, "k-mer sets").  km_check_pairs is what stands between such a file and the table the correction kernels
// read: one streaming pass over a slab of n pairs (12 bytes a pair) that
//   - judges every pair: keys[i] > keys[i - 1] (the slab's first key against `prev`, the last key of the slab before, when
//     there is one), keys[i] < 4^k, keys[i] <= its reverse complement (canonical), counts[i] >= keep -- the first rule a pair
//     breaks, in that order, is its reason (KM_CHECK_*);
//   - adds the keys and the counts up, modulo 2^64: per thread, per wave (shuffles), per workgroup (LDS), then ONE atomic a
//     sum and workgroup;
//   - keeps the lowest offender: ((first + i) << 3) | reason, reduced the same way with min, so the word names the lowest
//     global pair index that breaks a rule whatever the thread order.
// A thread takes two neighbouring pairs a step: the keys as one 16-byte load and the counts as one 8-byte load where the arrays
// are aligned for it (VEC; the launcher decides), plain loads otherwise and for an odd last pair.  The key before a thread's
// first pair is one more 8-byte load, of a line a neighbouring thread loads anyway.  Plain vector loads and ordinary atomics only.
#pragma once
#include "kbbq_kmer.h"

constexpr u64 KM_CHECK_NONE = ~0ull;
constexpr u32 KM_CHECK_ORDER = 1, KM_CHECK_RANGE = 2, KM_CHECK_CANONICAL = 3, KM_CHECK_COUNT = 4;

struct KmerCheck {
    const u64* keys; const u32* counts; int64_t n;
    int64_t first;                    // global index of the slab's pair 0 (what an offender is reported as)
    u64 prev; u32 have_prev;          // the key before the slab's first, when the slab is not the file's first
    int k; u32 keep;
    u64* out;                         // [0] += sum of keys, [1] += sum of counts, [2] = min(offender word)
};

__device__ __forceinline__ u32 km_check_pair(const KmerCheck& q, u64 limit, u64 key, u32 count, u64 before, bool has_before)
{
    if (has_before && key <= before) return KM_CHECK_ORDER;
    if (limit && key >= limit) return KM_CHECK_RANGE;
    if (key > km_revcomp(key, q.k)) return KM_CHECK_CANONICAL;
    if (count < q.keep) return KM_CHECK_COUNT;
    return 0;
}

template <bool VEC>
__global__ __launch_bounds__(KM_THREADS) void km_check_pairs(KmerCheck q)
{
    __shared__ u64 part[3][KM_THREADS / 64];
    const u64 limit = q.k < 32 ? 1ull << (2 * q.k) : 0;               // k = 32: every 64-bit word is in range
    u64 ksum = 0, csum = 0, bad = KM_CHECK_NONE;
    const int64_t steps = (q.n + 1) / 2;
    const int64_t stride = (int64_t)gridDim.x * KM_THREADS;
    for (int64_t s = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; s < steps; s += stride) {
        const int64_t i = 2 * s;
        const bool two = i + 1 < q.n;
        u64 k0, k1 = 0; u32 c0, c1 = 0;
        if (VEC && two) {
            const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(q.keys + i);
            const uint2 cc = *reinterpret_cast<const uint2*>(q.counts + i);
            k0 = kk.x; k1 = kk.y; c0 = cc.x; c1 = cc.y;
        } else {
            k0 = q.keys[i]; c0 = q.counts[i];
            if (two) { k1 = q.keys[i + 1]; c1 = q.counts[i + 1]; }
        }
        const u64 before = i ? q.keys[i - 1] : q.prev;
        u32 why = km_check_pair(q, limit, k0, c0, before, i ? true : q.have_prev != 0);
        if (why) bad = min(bad, ((u64)(q.first + i) << 3) | why);
        ksum += k0; csum += c0;
        if (two) {
            why = km_check_pair(q, limit, k1, c1, k0, true);
            if (why) bad = min(bad, ((u64)(q.first + i + 1) << 3) | why);
            ksum += k1; csum += c1;
        }
    }
    #pragma unroll
    for (int d = 32; d; d >>= 1) {
        ksum += __shfl_down(ksum, d, 64);
        csum += __shfl_down(csum, d, 64);
        bad = min(bad, (u64)__shfl_down(bad, d, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = ksum; part[1][wave] = csum; part[2][wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < KM_THREADS / 64; ++w) { ksum += part[0][w]; csum += part[1][w]; bad = min(bad, part[2][w]); }
        if (ksum) atomicAdd(q.out + 0, ksum);
        if (csum) atomicAdd(q.out + 1, csum);
        if (bad != KM_CHECK_NONE) atomicMin(q.out + 2, bad);
    }
}
