// kbbq_bam_index.h -- --bam-index: what a BAI / CSI index needs of a slab of --bam-out records, reduced where the records are
// assembled (include/kbbq_hip.h "BAM index", kbbq/_bamindex.py).
//
// The skeleton the assemble kernel reads holds every record's fixed fields and CIGAR, the descriptors hold the records' offsets in
// the uncompressed stream.  bi_entry is the one statement of what a record gives the index -- refID, [beg, end), its bin
// (reg2bin at 14 + 3 * depth bits: the record's own bin field only covers depth 5), its [start, start + length) in the stream --
// compiled for the device (kbi_entries: one lane per record) and for the host (kbbq_bam_index).  Absolute stream offsets are monotone
// in virtual file offsets, so every reduction here is in stream offsets and the host converts what is left.
//
//   kbi_entries   one lane per record: its key (refID, unmapped, bin) and length into scratch; a 64-bit atomicMin of its start
//                 into every 16 kb window of the file-long linear array it overlaps (the window clamped to the reference's last)
//   kbi_count     head flags ((refID, bin) differs from the predecessor's) and unmapped flags, counted by wave64 ballots: a pair
//                 of totals per workgroup
//   kbi_scan      one workgroup: the exclusive scan of those pairs, the grand totals
//   kbi_heads     every head's row and the unmapped records before it, compacted to the head's rank
//   kbi_runs      one lane per run: {refID, bin, beg, end, n_mapped, n_unmapped}, 32 bytes -- all that goes back to the host
//
// A record that does not fit (a head outside the skeleton, a CIGAR outside the head, a refID beyond the references, an end beyond
// 2^(14 + 3 * depth)) touches no window; the lowest such row is reported and the runs are not used.  Plain C++: vector stores,
// ordinary atomics.
#pragma once
#include "../../include/kbbq_hip.h"
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BI_HD __host__ __device__ __forceinline__
#else
#define BI_HD inline
#endif

constexpr int BIX_THREADS = 256;
constexpr int BIX_MIN_SHIFT = 14;
constexpr uint64_t BIX_UNMAPPED = 1ull << 31;            // bit 31 of a key: flag 4; the rest: refID << 32 | bin
constexpr uint64_t BIX_RUN_MASK = ~BIX_UNMAPPED;         // what decides a run: (refID, bin)
constexpr uint64_t BIX_NO_FIT = ~0ull;                   // the key of a record that does not fit

struct BixEntry {
    int32_t ref;                                         // -1: no coordinate
    uint32_t bin, length;                                // length: 4 + block_size, the record's bytes of the stream
    bool unmapped;
    int64_t beg, end;
};

// SAM specification 5.3 / the CSI specification: the smallest bin that holds [beg, end)
BI_HD uint32_t bix_reg2bin(int64_t beg, int64_t end, int depth)
{
    int s = BIX_MIN_SHIFT;
    uint32_t t = ((1u << (depth * 3)) - 1) / 7;
    --end;
    for (int l = depth; l > 0; --l, s += 3, t -= 1u << (l * 3))
        if (beg >> s == end >> s) return t + (uint32_t)(beg >> s);
    return 0;
}

BI_HD uint32_t bix_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
BI_HD uint32_t bix_u16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// One record, from its head in the skeleton (unaligned: byte loads).  false: it does not fit.
BI_HD bool bix_entry(const kbbq_bam_desc& d, const uint8_t* skel, uint64_t skel_bytes, int depth, int n_ref, BixEntry& e)
{
    if (d.head_bytes < 36 || (uint64_t)d.skel_off + d.head_bytes > skel_bytes) return false;
    const uint8_t* h = skel + d.skel_off;
    const uint32_t l_name = h[12], n_cigar = bix_u16(h + 16), flag = bix_u16(h + 18);
    if (36ull + l_name + 4ull * n_cigar > d.head_bytes) return false;
    const int32_t ref = (int32_t)bix_u32(h + 4), pos = (int32_t)bix_u32(h + 8);
    e.length = 4 + bix_u32(h);
    e.unmapped = (flag & 4) != 0;
    if (ref < 0) { e.ref = -1; e.bin = 0; e.beg = e.end = 0; return true; }
    if (ref >= n_ref) return false;
    int64_t span = 0;
    if (!e.unmapped) {
        const uint8_t* c = h + 36 + l_name;
        for (uint32_t k = 0; k < n_cigar; ++k, c += 4) {
            const uint32_t w = bix_u32(c), op = w & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += w >> 4;        // M D N = X
        }
    }
    e.ref = ref;
    e.beg = pos < 0 ? 0 : pos;
    e.end = e.beg + (span > 1 ? span : 1);
    if (e.end > (int64_t)1 << (BIX_MIN_SHIFT + 3 * depth)) return false;
    e.bin = bix_reg2bin(e.beg, e.end, depth);
    return true;
}

BI_HD uint64_t bix_key(const BixEntry& e) { return (uint64_t)(uint32_t)e.ref << 32 | (e.unmapped ? BIX_UNMAPPED : 0) | e.bin; }

// the windows of the linear array [beg >> 14, (end - 1) >> 14] of reference e.ref, clamped to its last: min(start) into each
template <class Min> BI_HD void bix_windows(const BixEntry& e, const uint64_t* lin_off, uint64_t start, const Min& put)
{
    const uint64_t base = lin_off[e.ref];
    if (lin_off[e.ref + 1] <= base) return;                                                  // (every reference has >= 2 windows)
    const uint64_t last = lin_off[e.ref + 1] - base - 1;
    uint64_t w = (uint64_t)e.beg >> BIX_MIN_SHIFT;
    const uint64_t hi = (uint64_t)(e.end - 1) >> BIX_MIN_SHIFT;
    for (; w <= hi && w < last; ++w) put(base + w, start);
    if (w <= hi) put(base + last, start);
}

#if defined(__HIPCC__)
struct BixParams {
    const uint8_t* skel; const kbbq_bam_desc* desc; const uint64_t* lin_off; uint64_t* linear;
    uint64_t skel_bytes, stream_base, lin_total;
    uint32_t n, n_ref; int depth;
    uint64_t* key;                                       // [n]
    uint32_t* length;                                    // [n]
    uint2* block;                                        // [ceil(n / BIX_THREADS)] (heads, unmapped) of a workgroup, then their scan
    uint32_t* head_row; uint32_t* head_unm;              // [n] per run: its first row, the unmapped records before it
    kbbq_bam_run* runs;                                  // [n]
    uint32_t* words;                                     // [0] the lowest row that does not fit, [1] runs, [2] unmapped records
};

struct BixAtomicMin {
    uint64_t* linear; uint64_t total;
    __device__ void operator()(uint64_t at, uint64_t v) const
    {
        if (at < total) atomicMin(reinterpret_cast<unsigned long long*>(linear + at), (unsigned long long)v);
    }
};

__global__ __launch_bounds__(BIX_THREADS) void kbi_entries(BixParams p)
{
    const uint32_t r = blockIdx.x * BIX_THREADS + threadIdx.x;
    if (r >= p.n) return;
    const kbbq_bam_desc d = p.desc[r];
    BixEntry e;
    if (!bix_entry(d, p.skel, p.skel_bytes, p.depth, (int)p.n_ref, e)) {
        p.key[r] = BIX_NO_FIT;
        p.length[r] = 0;
        atomicMin(&p.words[0], r);
        return;
    }
    p.key[r] = bix_key(e);
    p.length[r] = e.length;
    if (e.ref >= 0) bix_windows(e, p.lin_off, p.stream_base + d.stream_off, BixAtomicMin{p.linear, p.lin_total});
}

// (head, unmapped with a coordinate) of row r
__device__ __forceinline__ void bix_flags(const BixParams& p, uint32_t r, bool& head, bool& unm)
{
    head = unm = false;
    if (r >= p.n) return;
    const uint64_t k = p.key[r];
    head = r == 0 || ((k ^ p.key[r - 1]) & BIX_RUN_MASK) != 0;
    unm = (k & BIX_UNMAPPED) != 0 && k != BIX_NO_FIT;
}

__global__ __launch_bounds__(BIX_THREADS) void kbi_count(BixParams p)
{
    __shared__ uint32_t heads[BIX_THREADS / 64], unms[BIX_THREADS / 64];
    bool head, unm;
    bix_flags(p, blockIdx.x * BIX_THREADS + threadIdx.x, head, unm);
    const uint64_t hb = __ballot(head), ub = __ballot(unm);
    if ((threadIdx.x & 63) == 0) { heads[threadIdx.x >> 6] = (uint32_t)__popcll(hb); unms[threadIdx.x >> 6] = (uint32_t)__popcll(ub); }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 t = make_uint2(0, 0);
        for (int w = 0; w < BIX_THREADS / 64; ++w) { t.x += heads[w]; t.y += unms[w]; }
        p.block[blockIdx.x] = t;
    }
}

// one workgroup: block[] <- its exclusive scan; words[1], words[2] <- the totals
__global__ __launch_bounds__(BIX_THREADS) void kbi_scan(BixParams p, uint32_t nblocks)
{
    __shared__ uint2 part[BIX_THREADS];
    const uint32_t per = (nblocks + BIX_THREADS - 1) / BIX_THREADS;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
    uint2 sum = make_uint2(0, 0);
    for (uint32_t b = lo; b < hi; ++b) { const uint2 v = p.block[b]; sum.x += v.x; sum.y += v.y; }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 run = make_uint2(0, 0);
        for (int t = 0; t < BIX_THREADS; ++t) { const uint2 v = part[t]; part[t] = run; run.x += v.x; run.y += v.y; }
        p.words[1] = run.x;
        p.words[2] = run.y;
    }
    __syncthreads();
    uint2 run = part[threadIdx.x];
    for (uint32_t b = lo; b < hi; ++b) { const uint2 v = p.block[b]; p.block[b] = run; run.x += v.x; run.y += v.y; }
}

__global__ __launch_bounds__(BIX_THREADS) void kbi_heads(BixParams p)
{
    __shared__ uint32_t heads[BIX_THREADS / 64], unms[BIX_THREADS / 64];
    const uint32_t r = blockIdx.x * BIX_THREADS + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    bool head, unm;
    bix_flags(p, r, head, unm);
    const uint64_t hb = __ballot(head), ub = __ballot(unm), below = (1ull << lane) - 1;
    if (lane == 0) { heads[wave] = (uint32_t)__popcll(hb); unms[wave] = (uint32_t)__popcll(ub); }
    __syncthreads();
    if (!head) return;
    uint2 at = p.block[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) { at.x += heads[w]; at.y += unms[w]; }
    at.x += (uint32_t)__popcll(hb & below);
    at.y += (uint32_t)__popcll(ub & below);
    if (at.x < p.n) { p.head_row[at.x] = r; p.head_unm[at.x] = at.y; }
}

__global__ __launch_bounds__(BIX_THREADS) void kbi_runs(BixParams p)
{
    const uint32_t i = blockIdx.x * BIX_THREADS + threadIdx.x, count = p.words[1];
    if (i >= count || i >= p.n) return;
    const uint32_t r0 = p.head_row[i], last = i + 1 == count;
    const uint32_t r1 = last ? p.n : p.head_row[i + 1], u1 = last ? p.words[2] : p.head_unm[i + 1];
    if (r0 >= p.n || r1 > p.n || r1 <= r0) return;
    const uint64_t k = p.key[r0];
    kbbq_bam_run run;
    run.ref = (int32_t)(k >> 32);
    run.bin = (uint32_t)(k & 0x7FFFFFFFu);
    run.beg = p.stream_base + p.desc[r0].stream_off;
    run.end = p.stream_base + p.desc[r1 - 1].stream_off + p.length[r1 - 1];
    run.n_unmapped = u1 - p.head_unm[i];
    run.n_mapped = (r1 - r0) - run.n_unmapped;
    p.runs[i] = run;
}
#endif
