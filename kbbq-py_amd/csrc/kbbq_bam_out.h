// kbbq_bam_out.h -- --bam-out: the BAM stream of a slab of alignments, assembled where the apply kernel left its planes
// (include/kbbq_hip.h "BAM output", kbbq/_bamout.py).
//
// The host has written, per record, what it alone knows -- block_size, the 32 fixed bytes, QNAME, CIGAR, the encoded tags, the QUAL
// of a record the apply does not touch -- into a compact skeleton (csrc/sam_host.cpp kbbq_bam_skeleton) and a descriptor
// (kbbq_bam_desc).  A record of the stream is   head | SEQ, two characters to a byte | QUAL | tail   at the record's offset:
// head and tail come from the skeleton, SEQ from the character plane the apply read, QUAL from the apply's output plane (the
// character - 33) or, for a record whose QUAL stays as read, from the skeleton between head and tail.
//
// bo_record is the one statement of that, compiled for the device (kbo_assemble: BO_LANES lanes per record, BO_RECORDS records per
// workgroup) and for the host (kbbq_bam_assemble: one "lane").  A record of 150 bases is some 330 bytes -- twenty 16-byte pieces in
// four segments -- so a whole wave per record would leave three lanes in four idle; sixteen lanes take a segment in one or two
// steps, and the four records of a wave diverge only in their trip counts.  Rows of the planes are 16-byte aligned, destinations
// are not: every segment is written as single bytes up to the first 16-byte boundary of the DESTINATION, 16-byte stores from
// there, single bytes behind the last boundary; the sources of the 16-byte pieces are read at whatever alignment that leaves them
// (gfx950 reads a misaligned dwordx4 from global memory).  Plain C++ stores only.
#pragma once
#include "../../include/kbbq_hip.h"
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BO_HD __host__ __device__ __forceinline__
#else
#define BO_HD inline
#endif

constexpr int BO_THREADS = 256;                          // = the entries of the SEQ map: every thread stages one
constexpr int BO_LANES = 16;
constexpr int BO_RECORDS = BO_THREADS / BO_LANES;

struct alignas(16) bo_v16 { uint32_t w[4]; };

// SEQ character -> BAM nibble over "=ACMGRSVTWYHKDBN": lower case like upper case, anything else 15 (N)
BO_HD uint8_t bo_seq_code(uint32_t c)
{
    switch (c & ~0x20u) {                                // letters: the upper-case one ('=' is 0x3D: bit 5 is set in it)
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
        case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
        case 'D': return 13; case 'B': return 14; default: break;
    }
    if (c == '=') return 0;
    return 15;
}

// what a record needs of the buffers: is all of it inside them?
BO_HD bool bo_fits(const kbbq_bam_desc& d, uint64_t skel_bytes, uint64_t carry, uint64_t stream_bytes, uint32_t pitch)
{
    const uint64_t skel = (uint64_t)d.head_bytes + (d.qual_src == KBBQ_BAM_QUAL_SKELETON ? d.l_seq : 0u) + d.tail_bytes;
    const uint64_t rec = (uint64_t)d.head_bytes + ((uint64_t)d.l_seq + 1) / 2 + d.l_seq + d.tail_bytes;
    return d.l_seq <= pitch && d.qual_src <= KBBQ_BAM_QUAL_SKELETON && (uint64_t)d.skel_off + skel <= skel_bytes
           && carry + d.stream_off + rec <= stream_bytes;
}

// dst[0, n) <- op, by `nl` lanes of which this is `lane`
template <class Op> BO_HD void bo_segment(uint8_t* dst, uint32_t n, uint32_t lane, uint32_t nl, const Op& op)
{
    uint32_t lead = (uint32_t)(0 - (uintptr_t)dst) & 15u;
    if (lead > n) lead = n;
    const uint32_t mid = (n - lead) >> 4, rest = lead + (mid << 4);
    for (uint32_t j = lane; j < lead; j += nl) dst[j] = op.byte(j);
    for (uint32_t c = lane; c < mid; c += nl) {
        const uint32_t j = lead + (c << 4);
        bo_v16 v;
        op.vec(j, v);
        *reinterpret_cast<bo_v16*>(dst + j) = v;
    }
    for (uint32_t j = rest + lane; j < n; j += nl) dst[j] = op.byte(j);
}

struct BoCopy {                                          // skeleton bytes as they are
    const uint8_t* src;
    BO_HD uint8_t byte(uint32_t j) const { return src[j]; }
    BO_HD void vec(uint32_t j, bo_v16& v) const { memcpy(&v, src + j, 16); }
};

struct BoPack {                                          // two SEQ characters to a byte: byte j <- characters 2j, 2j + 1 (both exist)
    const uint8_t* seq; const uint8_t* map;
    BO_HD uint8_t byte(uint32_t j) const { return (uint8_t)(map[seq[2 * j]] << 4 | map[seq[2 * j + 1]]); }
    BO_HD void vec(uint32_t j, bo_v16& v) const
    {
        bo_v16 in[2];
        memcpy(in, seq + 2 * j, 32);
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = in[k >> 1].w[(k & 1) * 2], b = in[k >> 1].w[(k & 1) * 2 + 1];
            v.w[k] = (uint32_t)(map[a & 255] << 4 | map[(a >> 8) & 255]) | (uint32_t)(map[(a >> 16) & 255] << 4 | map[a >> 24]) << 8
                   | (uint32_t)(map[b & 255] << 4 | map[(b >> 8) & 255]) << 16 | (uint32_t)(map[(b >> 16) & 255] << 4 | map[b >> 24]) << 24;
        }
    }
};

struct BoQual {                                          // output characters - 33; *bad when one is below 33 (a quality below 0)
    const uint8_t* row; bool* bad;
    BO_HD uint8_t byte(uint32_t j) const { const uint8_t b = row[j]; if (b < 33) *bad = true; return (uint8_t)(b - 33); }
    BO_HD void vec(uint32_t j, bo_v16& v) const
    {
        memcpy(&v, row + j, 16);
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = v.w[k];
            // bit 7 of every byte: is the byte >= 33?  (its low seven bits + 95 carry into bit 7, or bit 7 is set already)
            const uint32_t ge = (((w & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) | w) & 0x80808080u;
            if (ge != 0x80808080u) *bad = true;
            v.w[k] = w - 0x21212121u;                    // no byte borrows from its neighbour when all are >= 33
        }
    }
};

// One record.  seq_row / out_row: the record's rows of the two planes (read only below l_seq); map: the 256 entries of
// bo_seq_code; stream: where stream offset 0 lies.  Returns whether this lane met a quality below 0.
BO_HD bool bo_record(const kbbq_bam_desc& d, const uint8_t* skel, const uint8_t* seq_row, const uint8_t* out_row, const uint8_t* map,
                     uint8_t* stream, uint32_t lane, uint32_t nl)
{
    const uint8_t* s = skel + d.skel_off;
    uint8_t* o = stream + d.stream_off;
    const uint32_t L = d.l_seq, pairs = L >> 1;
    bool bad = false;
    bo_segment(o, d.head_bytes, lane, nl, BoCopy{s});
    o += d.head_bytes; s += d.head_bytes;
    bo_segment(o, pairs, lane, nl, BoPack{seq_row, map});
    if ((L & 1) && lane == 0) o[pairs] = (uint8_t)(map[seq_row[L - 1]] << 4);       // the last nibble of an odd length is 0
    o += (L + 1) >> 1;
    if (d.qual_src == KBBQ_BAM_QUAL_SKELETON) { bo_segment(o, L, lane, nl, BoCopy{s}); s += L; }
    else {
        bo_segment(o, L, lane, nl, BoQual{out_row, &bad});
        // the SAM text of a one-base record whose new QUAL character is '*' says "no QUAL": the stream is that text's (lane 0 wrote o[0])
        if (L == 1 && lane == 0 && out_row[0] == '*') o[0] = 0xFF;
    }
    o += L;
    bo_segment(o, d.tail_bytes, lane, nl, BoCopy{s});
    return bad;
}

#if defined(__HIPCC__)
struct BoParams {
    const uint8_t* skel; const kbbq_bam_desc* desc; const uint8_t* seq; const uint8_t* out; uint8_t* stream;
    uint64_t skel_bytes, carry, stream_bytes;
    uint32_t n, pitch;
    uint32_t* words;                                     // [0] the lowest row with a quality below 0, [1] the lowest row that does not fit
};

__global__ __launch_bounds__(BO_THREADS) void kbo_assemble(BoParams p)
{
    __shared__ uint8_t map[BO_THREADS];
    map[threadIdx.x] = bo_seq_code(threadIdx.x);
    __syncthreads();
    const uint32_t r = blockIdx.x * BO_RECORDS + threadIdx.x / BO_LANES, lane = threadIdx.x % BO_LANES;
    if (r >= p.n) return;
    const kbbq_bam_desc d = p.desc[r];
    if (!bo_fits(d, p.skel_bytes, p.carry, p.stream_bytes, p.pitch)) {
        if (lane == 0) atomicMin(&p.words[1], r);
        return;
    }
    const size_t row = (size_t)r * p.pitch;
    if (bo_record(d, p.skel, p.seq + row, p.out + row, map, p.stream + p.carry, lane, BO_LANES)) atomicMin(&p.words[0], r);
}
#endif
